// dir_mano_fit_sequence: MANO fitted to whole sequences -- one shape per (sequence, hand), a pose and a camera per frame, neighbouring frames
// coupled in time.  The rule, the order of every operation and the status bits are written out in include/dir_hip.h ("MANO fitting: sequences").
//
// The coupling crosses workgroups, so unlike mano_fit.hip the iteration loop is on the HOST side of the launch: a launch boundary is the only
// synchronisation (no grid barrier, no flags).  The iterates live twice in the workspace; iteration k reads copy k & 1 (its own row and its two
// neighbours') and writes copy (k + 1) & 1, so every gradient is taken at iterate k.
//
//   mano_fit_seq_init_kernel     (N, hands)  classifies each frame (inert / no data), copies p0 into copy 0, finds the frame's sequence
//   mano_fit_seq_shape_kernel    (S, hands)  FIRST = true: the shared shape's start and prior centre; false: step 6, the fixed tree over the
//                                            frames' beta gradients and one Adam step on the shape
//   mano_fit_seq_kernel          (N, hands)  FINAL = false: one iteration of one frame, mano_fit_kernel's shape (256 threads, the hand in LDS, the two
//                                            schedules of mano_device.h; residuals, gradient tail and Adam of mano_fit_device.h); true: the forward-only
//                                            pass and mano_fit_device.h's output block
// The init kernel runs the target scan mano_fit_kernel runs, and the entry point the same checks of the options and the hands (mano_fit_device.h).
//
// fp32 throughout, every reduction in a fixed order, no atomics, nothing allocated: a sequence gives the same bits alone, in any slot of any ragged
// batch and in either hand slot.
#include "mano_fit_device.h"

namespace {

using namespace dir::mano;
using dir::finite;

constexpr int ST = DIR_MANO_FIT_STATE, SST = DIR_MANO_FIT_SEQ_STATE, RL = DIR_MANO_FIT_SEQ_LANES;
constexpr int F_INERT = 2, F_FROZEN = 4, F_NODATA = 8;

// the workspace, carved on the host: 4-byte items only, nothing read before a kernel of this call wrote it
struct SeqWork {
    float* P;            // [2][hands][N][64]   the two copies of the iterates
    float* state;        // [hands][N][ST]      the frames' Adam state where the caller gives none
    float* gb;           // [hands][N][10]      the frames' beta gradients of this iteration
    int32_t* flags;      // [hands][N]          F_*
    int32_t* seq_of;     // [N]
    float* sb;           // [hands][S][10]      the shared shapes
    float* sanchor;      // [hands][S][10]      their prior centres
    float* sstate;       // [hands][S][SST]     their Adam state where the caller gives none
    int32_t* sflags;     // [hands][S]
};
__host__ __device__ inline size_t work_items(size_t N, size_t S, size_t hands) {
    return hands * N * (2 * 64 + ST + 10 + 1) + N + hands * S * (10 + 10 + SST + 1);
}

struct SeqArgs {
    dir_mano_tables t[2];
    dir_mano_fit_hand h[2];
    float* state[2];                     // per hand: the caller's or the workspace's
    float* sstate[2];
    int own_state[2], own_sstate[2];     // the workspace's: the init kernels zero them
    SeqWork w;
    const int32_t* seq_start;
    int32_t* seq_status;
    fit::Rule r;
    float kt_root, kt_pca, kt_cam;       // 2 w_t_*
    int share, N, S, hands;
    int cur, first;                      // which copy holds the iterate that is read; the first iteration of the call (it writes mse before)
};

// the frames [s0, s1) of sequence s, clamped to the N frames whatever seq_start holds
__device__ __forceinline__ void seq_range(const SeqArgs& args, int s, int& s0, int& s1) {
    s0 = min(max(args.seq_start[s], 0), args.N);
    s1 = min(max(args.seq_start[s + 1], s0), args.N);
}

__global__ __launch_bounds__(BT) void mano_fit_seq_init_kernel(SeqArgs args) {
    const int h = blockIdx.y, tid = threadIdx.x;
    const dir_mano_fit_hand& a = args.h[h];
    const size_t b = blockIdx.x, row = (size_t)h * args.N + b;
    int bad_p = 0;
    if (tid < 64) {
        const float x = a.p0[b * 64 + tid];
        const float an = a.anchor ? a.anchor[b * 64 + tid] : x;
        args.w.P[row * 64 + tid] = x;                                   // copy 0
        bad_p = !finite(x) || !finite(an);
    }
    if (args.own_state[h])
        for (int i = tid; i < ST; i += BT) args.state[h][b * ST + i] = 0.f;
    const int bad_t = fit::targets_nonfinite(a, b, tid);
    const bool inert = __syncthreads_or(bad_p) != 0;
    const bool nodata = __syncthreads_or(bad_t) != 0;
    if (tid == 0) {
        args.w.flags[row] = inert ? F_INERT : nodata ? F_NODATA : 0;
        if (h == 0) {                                                   // the last sequence that starts at or before this frame
            int lo = 0, hi = args.S - 1;
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (args.seq_start[mid] <= (int)b) lo = mid; else hi = mid - 1;
            }
            args.w.seq_of[b] = lo;
        }
    }
}

// FIRST: the shape's start.  Otherwise step 6 of the rule.
template <bool FIRST> __global__ __launch_bounds__(RL) void mano_fit_seq_shape_kernel(SeqArgs args) {
    const int s = blockIdx.x, h = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t srow = (size_t)h * args.S + s;
    const dir_mano_fit_hand& a = args.h[h];
    int s0, s1;
    seq_range(args, s, s0, s1);
    if constexpr (FIRST) {
        __shared__ int s_first;
        if (tid == 0) {
            int f = -1;
            for (int n = s0; n < s1 && f < 0; ++n)
                if (!(args.w.flags[(size_t)h * args.N + n] & F_INERT)) f = n;
            s_first = f;
            args.w.sflags[srow] = f < 0 ? F_INERT : 0;
        }
        __syncthreads();
        const int f = s_first;
        if (tid < 10) {
            args.w.sb[srow * 10 + tid] = f < 0 ? 0.f : a.p0[(size_t)f * 64 + 51 + tid];
            args.w.sanchor[srow * 10 + tid] = f < 0 ? 0.f : (a.anchor ? a.anchor : a.p0)[(size_t)f * 64 + 51 + tid];
        }
        if (args.own_sstate[h] && tid < SST) args.sstate[h][(size_t)s * SST + tid] = 0.f;
    } else {
        __shared__ float s_part[RL / 64][10];
        const int sf = args.w.sflags[srow];
        if (sf & (F_INERT | F_FROZEN)) return;                          // no frame in a chain, or the shape is frozen (block-uniform)
        float acc[10] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int i = tid; i < s1 - s0; i += RL) {
            const size_t row = (size_t)h * args.N + s0 + i;
            const bool in = !(args.w.flags[row] & (F_INERT | F_FROZEN));
#pragma unroll
            for (int k = 0; k < 10; ++k) acc[k] += in ? args.w.gb[row * 10 + k] : 0.f;       // selected, never multiplied by 0
        }
#pragma unroll
        for (int k = 0; k < 10; ++k) { const float t = dir::wave_sum_dpp(acc[k]); if (lane == 0) s_part[wave][k] = t; }
        __syncthreads();
        float* st = args.sstate[h] + (size_t)s * SST;
        float b_new = 0.f, m_new = 0.f, v_new = 0.f, pb1n = 0.f, pb2n = 0.f;
        int bad = 0, t_step = 0;
        if (tid < 10) {
            t_step = __float_as_int(st[22]);
            const float pb1 = t_step > 0 ? st[20] : 1.f, pb2 = t_step > 0 ? st[21] : 1.f;
            pb1n = pb1 * args.r.b1; pb2n = pb2 * args.r.b2;
            float g = s_part[0][tid] + s_part[1][tid] + s_part[2][tid] + s_part[3][tid];
            b_new = args.w.sb[srow * 10 + tid];
            g = fit::prior_gradient(51 + tid, g, b_new, args.w.sanchor[srow * 10 + tid], args.r.k_pca, args.r.k_beta, args.r.k_init);
            m_new = st[tid]; v_new = st[10 + tid];
            bad = !fit::adam(g, args.r.lr[2], args.r.b1, args.r.b2, args.r.eps, pb1n, pb2n, b_new, m_new, v_new);
        }
        if (__syncthreads_or(bad)) {
            if (tid == 0) args.w.sflags[srow] = sf | F_FROZEN;
        } else if (tid < 10) {
            args.w.sb[srow * 10 + tid] = b_new; st[tid] = m_new; st[10 + tid] = v_new;
            if (tid == 0) { st[20] = pb1n; st[21] = pb2n; st[22] = __int_as_float(t_step + 1); st[23] = 0.f; }
        }
    }
}

template <bool FINAL> __global__ __launch_bounds__(BT) void mano_fit_seq_kernel(SeqArgs args) {
    const int hand = blockIdx.y;
    const dir_mano_tables& T = args.t[hand];
    const dir_mano_fit_hand& a = args.h[hand];
    const int side = T.side, center = T.center_idx, root_palm = T.root_palm;       // read once, here (mano_device.h, layer 2)
    __shared__ float s_v[NV3P];          // v_posed
    __shared__ float s_vert[NV3P];       // skinned vertices (before centring)
    __shared__ float s_gv[NV3P];         // g of the skinned vertices
    __shared__ float s_gvp[NV3P];        // g of v_posed (= g of v_shaped)
    __shared__ float s_p[64], s_anchor[64], s_m[64], s_vv[64], s_g[64];      // iterate, prior centre, Adam moments, gradient
    __shared__ float s_nb[2][64], s_nbR[2][9];                              // the neighbours t - 1, t + 1 at this iterate and their root rotations
    __shared__ float s_full[45];
    DIR_MANO_LDS(L, s);
    DIR_MANO_BWD_LDS(G, s);
    __shared__ float s_red[4][11], s_sum[11];
    __shared__ int s_flag;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = blockIdx.x, N = args.N;
    const size_t b = n, row = (size_t)hand * N + n;
    const float* s_pose = s_p;
    const float* s_beta = s_p + 51;
    const float* s_cam = s_p + 61;
    const int fl = args.w.flags[row];
    const bool inert = fl & F_INERT;
    const float* cur = args.w.P + ((size_t)args.cur * args.hands * N + row) * 64;
    float* nxt = args.w.P + ((size_t)(args.cur ^ 1) * args.hands * N + row) * 64;
    float* st = args.state[hand] + b * ST;
    const int seq = args.w.seq_of[n];
    const float* sb = args.w.sb + ((size_t)hand * args.S + seq) * 10;
    const bool share = args.share != 0;

    if constexpr (!FINAL) {
        if (inert) return;               // in no chain: nothing reads its rows (block-uniform, before any barrier)
        if (fl & F_FROZEN) {             // frozen: the iterate stays visible to the neighbours
            if (tid < 64) nxt[tid] = cur[tid];
            return;
        }
    }

    // ================================================================ the frame at this iterate, its state and its neighbours
    bool p0_bad = false;
    if constexpr (FINAL) {
        int bad_p = 0;
        if (tid < 64) {
            float x = inert ? a.p0[b * 64 + tid] : cur[tid];
            if (!inert && share && tid >= 51 && tid < 61) x = sb[tid - 51];
            s_p[tid] = x;
            bad_p = inert && !finite(x);
        }
        p0_bad = __syncthreads_or(bad_p) != 0;
    }
    float pb1 = 1.f, pb2 = 1.f;
    int t_step = 0;
    bool has[2] = {false, false};
    if constexpr (!FINAL) {
        fit::load_clock(st, 0, pb1, pb2, t_step);
        if (args.kt_root > 0.f || args.kt_pca > 0.f || args.kt_cam > 0.f) {
            int s0, s1;
            seq_range(args, seq, s0, s1);
            has[0] = n > s0 && n - 1 < s1 && !(args.w.flags[row - 1] & F_INERT);
            has[1] = n + 1 < s1 && n + 1 > s0 && !(args.w.flags[row + 1] & F_INERT);
        }
        if (tid < 64) {
            float x = cur[tid];
            if (share && tid >= 51 && tid < 61) x = sb[tid - 51];
            s_p[tid] = x;
            s_anchor[tid] = a.anchor ? a.anchor[b * 64 + tid] : a.p0[b * 64 + tid];
            s_m[tid] = st[tid];
            s_vv[tid] = st[64 + tid];
        } else if (tid < 192) {
            const int e = (tid >> 6) - 1;                                // 0: t - 1, 1: t + 1
            if (has[e]) s_nb[e][tid & 63] = (e ? cur + 64 : cur - 64)[tid & 63];
        }
        __syncthreads();
    }
    const bool data = !(fl & (F_INERT | F_NODATA));
    const bool use_v = a.verts_t && data, use_j = a.joints_t && data, use_uv = a.uv_t && data;

    // ================================================================ forward at s_p (mano_device.h, layers 2 and 4)
    if (tid < 45) s_full[tid] = pca_axis_angle(T, s_pose + 6, tid);
    shape_blend(T, s_beta, s_v, tid);
    if (tid == 64) { int reflect; robust6d(s_pose, L.root, reflect); s_flag = reflect; }
    if constexpr (!FINAL) {
        if ((tid == 65 || tid == 66) && has[tid - 65] && args.kt_root > 0.f) { int reflect; robust6d(s_nb[tid - 65], s_nbR[tid - 65], reflect); }
    }
    __syncthreads();
    forward_schedule(L, T, side, center, root_palm, s_full, s_beta, s_v, s_vert, tid);
    __syncthreads();

    // ================================================================ residuals: the cotangents gV, gJ, gU; the mean squared residuals at p0 and at the end
    const bool want_mse = FINAL || args.first;
    float red[11] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    fit::residuals(a, b, L, G, s_vert, s_gv, s_cam, use_v, use_j, use_uv, args.r.kv, args.r.kj, args.r.kuv, tid, red);
    fit::residual_partials(red, want_mse, s_red, lane, wave);
    if (tid < 48) { G.gAt[tid] = 0.f; }
    __syncthreads();
    if (tid < 11) s_sum[tid] = s_red[0][tid] + s_red[1][tid] + s_red[2][tid] + s_red[3][tid];
    __syncthreads();
    if (want_mse && tid < 3 && a.mse) {
        const float mse = p0_bad ? 0.f : fit::mean_sq(s_sum, use_v, tid);
        if (!FINAL || inert || args.r.iters == 0) a.mse[b * 6 + tid] = mse;      // at p0: the first iteration wrote it for the frames that step
        if (FINAL) a.mse[b * 6 + 3 + tid] = mse;
    }

    if constexpr (FINAL) {
        // ================================================================ outputs at the final iterate
        fit::write_outputs(a, b, L, s_vert, s_cam, p0_bad, tid);
        if (tid < 64) a.p_out[b * 64 + tid] = s_p[tid];
        if (tid == 64 && a.status) a.status[b] = fl | (p0_bad ? 0 : s_flag);
        if (tid == 66 && !inert && __float_as_int(st[130]) == 0) { st[128] = 1.f; st[129] = 1.f; st[131] = 0.f; }      // no step taken: the state dir_mano_fit returns, P1 = P2 = 1
        if (tid == 65 && hand == 0 && n < args.S && args.seq_status)
            for (int hh = 0; hh < args.hands; ++hh) args.seq_status[(size_t)hh * args.S + n] = args.w.sflags[(size_t)hh * args.S + n];
    } else {
        // ================================================================ backward (mano_device.h, layers 3 and 4), the gradient into s_g
        DIR_MANO_BACKWARD_SCHEDULE(dir::wave_sum_dpp, G, L, T, side, center, root_palm, s_sum, s_v, s_gv, s_gvp, tid);
        rodrigues_bwd(G, L, s_full, tid);
        if (tid == 64) {
            if (args.kt_root > 0.f) {                                    // the temporal root term, on the 3x3 cotangent: t - 1 first, then t + 1
#pragma clang fp contract(off)
                for (int e = 0; e < 2; ++e)
                    if (has[e])
                        for (int i = 0; i < 9; ++i) G.groot[i] = G.groot[i] + args.kt_root * (L.root[i] - s_nbR[e][i]);
            }
            robust6d_bwd(s_pose, G.groot, s_g);
        }
        fit::gradient_tail(G, T, s_gvp, s_sum, s_g, tid);
        __syncthreads();
        if (tid < 45) s_g[6 + tid] = pca_bwd(G, T, tid);
        __syncthreads();

        // ================================================================ the priors' and the temporal gradients, one Adam step (include/dir_hip.h gives this order)
        float p_new = 0.f, m_new = 0.f, v_new = 0.f;
        int bad = 0;
        const float pb1n = pb1 * args.r.b1, pb2n = pb2 * args.r.b2;
        const bool shared_comp = share && tid >= 51 && tid < 61;          // the shape's step is mano_fit_seq_shape_kernel's
        if (tid < 64) {
            const float p = s_p[tid];
            p_new = p; m_new = s_m[tid]; v_new = s_vv[tid];
            if (shared_comp) {
                args.w.gb[row * 10 + tid - 51] = s_g[tid];
            } else {
                float g = fit::prior_gradient(tid, s_g[tid], p, s_anchor[tid], args.r.k_pca, args.r.k_beta, args.r.k_init);
                const float kt = tid >= 6 && tid < 51 ? args.kt_pca : tid >= 61 ? args.kt_cam : 0.f;
                if (kt > 0.f) {
#pragma clang fp contract(off)
                    if (has[0]) g = g + kt * (p - s_nb[0][tid]);
                    if (has[1]) g = g + kt * (p - s_nb[1][tid]);
                }
                bad = !fit::adam(g, args.r.lr[fit::group_of(tid)], args.r.b1, args.r.b2, args.r.eps, pb1n, pb2n, p_new, m_new, v_new);
            }
        }
        if (__syncthreads_or(bad)) {          // the step is not taken: the frame is frozen at this iterate, its state stays
            if (tid < 64) nxt[tid] = cur[tid];
            if (tid == 64) args.w.flags[row] = fl | F_FROZEN;
        } else {
            if (tid < 64) {
                nxt[tid] = shared_comp ? cur[tid] : p_new;
                if (!shared_comp) { st[tid] = m_new; st[64 + tid] = v_new; }
            }
            if (tid == 64) fit::store_clock(st, 0, pb1n, pb2n, t_step + 1);
        }
    }
}

}  // namespace

extern "C" size_t dir_mano_fit_sequence_workspace_bytes(int N, int S, int hands) {
    if (N <= 0 || S <= 0 || S > N || (hands != 1 && hands != 2)) return 0;
    return 4 * work_items(N, S, hands);
}

extern "C" int dir_mano_fit_sequence(const dir_mano_tables* tables_host, const dir_mano_fit_hand* hands_host, const dir_mano_fit_opts* opts_host,
                                     const dir_mano_fit_seq_opts* seq_opts_host, const int32_t* seq_start, int S, int N, int hands,
                                     int32_t* seq_status, void* work, size_t work_bytes, void* stream) {
    using namespace dir;
    if (N == 0 && S == 0) return DIR_OK;
    DIR_REQUIRE(N > 0 && S > 0 && S <= N && (hands == 1 || hands == 2) && tables_host && hands_host && opts_host && seq_opts_host && seq_start,
                "dir_mano_fit_sequence: bad arguments");
    const dir_mano_fit_seq_opts& q = *seq_opts_host;
    SeqArgs a;
    if (int rc = mano::fit::check_opts(*opts_host, {q.w_t_root, q.w_t_pca, q.w_t_cam}, "dir_mano_fit_sequence", a.r)) return rc;
    DIR_REQUIRE(work && ((uintptr_t)work & 3) == 0 && work_bytes >= dir_mano_fit_sequence_workspace_bytes(N, S, hands),
                "dir_mano_fit_sequence: workspace too small (or null, or not 4-byte aligned)");
    if (q.seq_start_host) {
        DIR_REQUIRE(q.seq_start_host[0] == 0 && q.seq_start_host[S] == N, "dir_mano_fit_sequence: seq_start must run from 0 to N");
        for (int s = 0; s < S; ++s) DIR_REQUIRE(q.seq_start_host[s] <= q.seq_start_host[s + 1], "dir_mano_fit_sequence: seq_start must ascend");
    }
    const size_t n = N, s = S, hn = (size_t)hands * n, hs = (size_t)hands * s;
    float* w = (float*)work;
    a.w.P = w; w += 2 * hn * 64;
    a.w.state = w; w += hn * ST;
    a.w.gb = w; w += hn * 10;
    a.w.flags = (int32_t*)w; w += hn;
    a.w.seq_of = (int32_t*)w; w += n;
    a.w.sb = w; w += hs * 10;
    a.w.sanchor = w; w += hs * 10;
    a.w.sstate = w; w += hs * SST;
    a.w.sflags = (int32_t*)w;
    for (int h = 0; h < hands; ++h) {
        const dir_mano_tables& t = tables_host[h];
        if (int rc = mano::check_mano_tables(t, "dir_mano_fit_sequence")) return rc;
        const dir_mano_fit_hand& f = hands_host[h];
        if (int rc = mano::fit::check_hand(f, "dir_mano_fit_sequence")) return rc;
        a.t[h] = t;
        a.h[h] = f;
        a.own_state[h] = !f.state; a.state[h] = f.state ? f.state : a.w.state + (size_t)h * n * ST;
        a.own_sstate[h] = !q.seq_state[h]; a.sstate[h] = q.seq_state[h] ? q.seq_state[h] : a.w.sstate + (size_t)h * s * SST;
    }
    if (hands == 1) { a.t[1] = a.t[0]; a.h[1] = a.h[0]; a.state[1] = a.state[0]; a.sstate[1] = a.sstate[0]; a.own_state[1] = a.own_state[0]; a.own_sstate[1] = a.own_sstate[0]; }
    a.seq_start = seq_start; a.seq_status = seq_status;
    a.kt_root = 2.f * q.w_t_root; a.kt_pca = 2.f * q.w_t_pca; a.kt_cam = 2.f * q.w_t_cam;
    a.share = q.share_betas != 0; a.N = N; a.S = S; a.hands = hands; a.cur = 0; a.first = 0;
    hipStream_t st = (hipStream_t)stream;
    DIR_LAUNCH(mano_fit_seq_init_kernel, dim3(N, hands), dim3(BT), 0, st, a);
    DIR_LAUNCH(mano_fit_seq_shape_kernel<true>, dim3(S, hands), dim3(RL), 0, st, a);
    for (int it = 0; it < a.r.iters; ++it) {
        a.cur = it & 1; a.first = it == 0;
        DIR_LAUNCH(mano_fit_seq_kernel<false>, dim3(N, hands), dim3(BT), 0, st, a);
        if (a.share) DIR_LAUNCH(mano_fit_seq_shape_kernel<false>, dim3(S, hands), dim3(RL), 0, st, a);
    }
    a.cur = a.r.iters & 1; a.first = 0;
    DIR_LAUNCH(mano_fit_seq_kernel<true>, dim3(N, hands), dim3(BT), 0, st, a);
    return check_launch("dir_mano_fit_sequence");
}
