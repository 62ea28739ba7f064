// dir_mano_fit_pair: the two hands of a pair fitted TOGETHER -- dir_mano_fit's energy for each hand, the offset o between their centre joints as a
// further variable, and a capsule-per-bone collision term between them.  The rule, the order of every operation and the status bits are written
// out in include/dir_hip.h ("MANO fitting: two hands together"); tests/helpers/mano_pair_fit_ref.py restates it in torch.
//
// One 512-thread workgroup per pair: threads 0-255 run the left slot and 256-511 the right through the SAME schedules and fit pieces mano_fit_kernel
// runs (mano_device.h / mano_fit_device.h, with the thread index taken modulo 256), each on its own set of LDS arrays; the barriers are workgroup wide,
// so after centre() both hands' joints of the same iterate are in LDS.  40 threads (one bone of one hand each) then walk the other hand's 20 bones
// in order, 42 threads gather the bones' sums into the joint cotangents, and both backwards run.  No recomputed forward, no traffic between
// workgroups, no atomics.  Where no capsule pair is active nothing is added, and both hands get dir_mano_fit's bits.
#include "bone_common.h"
#include "mano_fit_device.h"

namespace {

using namespace dir::mano;
using dir::finite;
using dir::bone::kChild;
using dir::bone::kParent;

constexpr int OST = DIR_MANO_FIT_PAIR_STATE;
constexpr int PT = 2 * BT;               // the pair's workgroup

struct PairArgs {
    dir_mano_tables t[2];
    dir_mano_fit_hand h[2];
    dir_mano_fit_pair_args p;
    fit::Rule r;                         // as mano_fit.hip's
    float k_col, k_off, k_oi, lr_o;      // 2 w_col / 400 (formed in double, rounded once), 2 w_off, 2 w_off_init
};

__global__ __launch_bounds__(PT) void mano_fit_pair_kernel(PairArgs args) {
    // `hand` is the same for the 64 lanes of a wave: read as a scalar, so the tables, the row's pointers and the LDS bases it selects stay in SGPRs.
    // `lt` is made opaque at the top of every iteration, so the addresses derived from it are formed where they are used and not kept live across
    // the loop: together 692 -> 72 bytes of scratch per lane under the 256 VGPRs that 512 threads leave ("MANO fitting: two hands together").
    const int tid = threadIdx.x, hand = __builtin_amdgcn_readfirstlane(tid >> 8);
    int lt = tid & (BT - 1), lane = lt & 63, wave = lt >> 6;
    const dir_mano_tables& T = args.t[hand];
    const dir_mano_fit_hand& a = args.h[hand];
    const dir_mano_fit_pair_args& pa = args.p;
    const int side = T.side, center = T.center_idx, root_palm = T.root_palm;
    __shared__ float s_v2[2][NV3P], s_vert2[2][NV3P], s_gv2[2][NV3P], s_gvp2[2][NV3P];
    __shared__ float s_p2[2][64], s_p02[2][64], s_anchor2[2][64], s_m2[2][64], s_vv2[2][64], s_g2[2][64];
    __shared__ float s_full2[2][45];
    __shared__ float s_rot[2][135], s_pm[2][135], s_root[2][9], s_J[2][48], s_A[2][NJ * 12], s_jtr[2][63], s_c[2][3];
    __shared__ __attribute__((aligned(16))) float s_A2[2][NJ * 12];
    __shared__ float s_gj[2][63], s_gAt[2][48], s_gA2[2][NJ * 12], s_gA[2][NJ * 12], s_gJ[2][48], s_gR[2][135], s_gfull[2][45], s_part[2][5][15], s_groot[2][9];
    __shared__ float s_red2[2][4][11], s_sum2[2][11], s_mse2[2][6];
    __shared__ int s_flag2[2];
    // the pair's own: o, its start / anchor / target / moments, the radii, the joints in the common frame, and the bones' sums
    __shared__ float s_o[3], s_o0[3], s_oa[3], s_ot[3], s_om[3], s_ov[3], s_rad[2][20];
    __shared__ float s_x[2][63];                     // X^L = J^L, X^R = J^R + o
    __shared__ float s_bone[2][20][6];               // parent-end sum | child-end sum of one bone
    __shared__ int s_bact[2][20];                    // the bone has an active pair
    __shared__ float s_rowe[20], s_rowm[20], s_rowgo[20][3];
    __shared__ int s_nodir[20];
    __shared__ float s_col[4], s_go[3];

    const Lds L = {s_A2[hand], s_rot[hand], s_pm[hand], s_root[hand], s_J[hand], s_A[hand], s_jtr[hand], s_c[hand]};
    const BwdLds G = {s_gj[hand], s_gAt[hand], s_gA2[hand], s_gA[hand], s_gJ[hand], s_gR[hand], s_gfull[hand], s_part[hand], s_groot[hand]};
    float* const s_v = s_v2[hand]; float* const s_vert = s_vert2[hand]; float* const s_gv = s_gv2[hand]; float* const s_gvp = s_gvp2[hand];
    float* const s_p = s_p2[hand]; float* const s_p0 = s_p02[hand]; float* const s_anchor = s_anchor2[hand];
    float* const s_m = s_m2[hand]; float* const s_vv = s_vv2[hand]; float* const s_g = s_g2[hand]; float* const s_full = s_full2[hand];
    float (*const s_red)[11] = s_red2[hand];
    float* const s_sum = s_sum2[hand]; float* const s_mse = s_mse2[hand];

    const size_t b = blockIdx.x;
    const float* s_pose = s_p;
    const float* s_beta = s_p + 51;
    const float* s_cam = s_p + 61;

    // ================================================================ start: each hand's row as mano_fit_kernel reads it, then o and the radii
    float pb1, pb2;                      // this hand's b1^t, b2^t
    int t_step;
    fit::load_clock(a.state, b, pb1, pb2, t_step);
    float po1 = 1.f, po2 = 1.f;          // o's
    int t_o = 0;
    if (pa.o_state) {
        t_o = __float_as_int(pa.o_state[b * OST + 8]);
        if (t_o > 0) { po1 = pa.o_state[b * OST + 6]; po2 = pa.o_state[b * OST + 7]; }
    }
    const int bad_p = fit::load_row(a, b, s_p0, s_p, s_anchor, s_m, s_vv, lt);
    const int bad_t = fit::targets_nonfinite(a, b, lt);
    int bad_o = 0;
    const float c_o = pa.o_target ? (pa.o_conf ? pa.o_conf[b] : 1.f) : 0.f;
    const bool use_ot = c_o > 0.f;                    // selected, never multiplied by 0
    if (lt >= 64 && lt < 84) {
        const float r = pa.radii[hand][lt - 64];
        s_rad[hand][lt - 64] = r;
        bad_o |= !finite(r);
    }
    if (tid >= 96 && tid < 99) {
        const int c = tid - 96;
        const float x = pa.o0[b * 3 + c], an = pa.o_anchor ? pa.o_anchor[b * 3 + c] : x, tg = use_ot ? pa.o_target[b * 3 + c] : 0.f;
        s_o0[c] = x; s_o[c] = x; s_oa[c] = an; s_ot[c] = tg;
        s_om[c] = pa.o_state ? pa.o_state[b * OST + c] : 0.f;
        s_ov[c] = pa.o_state ? pa.o_state[b * OST + 3 + c] : 0.f;
        bad_o |= !finite(x) || !finite(an) || !finite(tg) || (use_ot && !finite(c_o));
    }
    // (__syncthreads_or returns whether ANY thread's predicate is set, not the bitwise OR: one call per flag)
    const bool p0_bad_l = __syncthreads_or(bad_p && hand == 0) != 0, p0_bad_r = __syncthreads_or(bad_p && hand == 1) != 0;
    const bool pass_l = __syncthreads_or(bad_t && hand == 0) != 0 || p0_bad_l, pass_r = __syncthreads_or(bad_t && hand == 1) != 0 || p0_bad_r;
    const bool o_bad = __syncthreads_or(bad_o) != 0;
    const bool p0_bad = hand ? p0_bad_r : p0_bad_l;
    const bool pass = hand ? pass_r : pass_l;                           // this hand passes through
    const bool any_pass = pass_l || pass_r;
    const bool coupled = !any_pass && !o_bad;                           // uniform over the workgroup
    const bool use_v = a.verts_t && !pass, use_j = a.joints_t && !pass, use_uv = a.uv_t && !pass;
    bool alive = !pass, other_alive = !(hand ? pass_l : pass_r), o_alive = coupled;
    int status = pass ? 2 : 0;
    int pstatus = (any_pass ? 1 : 0) | (o_bad ? 2 : 0);
    const bool grad_col = coupled && args.k_col > 0.f;

    for (int it = 0;; ++it) {
        asm volatile("" : "+v"(lt));
        lane = lt & 63; wave = lt >> 6;
        // ================================================================ forward at s_p (mano_device.h, layers 2 and 4)
        if (lt < 45) s_full[lt] = pca_axis_angle(T, s_pose + 6, lt);
        shape_blend(T, s_beta, s_v, lt);
        if (lt == 64) { int reflect; robust6d(s_pose, L.root, reflect); s_flag2[hand] = reflect; }
        __syncthreads();
        forward_schedule(L, T, side, center, root_palm, s_full, s_beta, s_v, s_vert, lt);
        __syncthreads();

        // ================================================================ residuals of each hand; the joints in the common frame
        const bool last = it >= args.r.iters || !(alive || other_alive || o_alive);       // uniform
        const bool want_mse = it == 0 || last;
        const bool run_col = coupled && (want_mse || (grad_col && !last));
        float red[11] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        fit::residuals(a, b, L, G, s_vert, s_gv, s_cam, use_v, use_j, use_uv, args.r.kv, args.r.kj, args.r.kuv, lt, red);
        fit::residual_partials(red, want_mse, s_red, lane, wave);
        if (lt < 48) { G.gAt[lt] = 0.f; }
        if (run_col && lt >= 64 && lt < 64 + 63) {
#pragma clang fp contract(off)
            const int i = lt - 64;
            const float x = L.jtr[i] - L.c[i % 3];
            s_x[hand][i] = hand ? x + s_o[i % 3] : x;
        }
        __syncthreads();
        if (lt < 11) s_sum[lt] = s_red[0][lt] + s_red[1][lt] + s_red[2][lt] + s_red[3][lt];
        // ================================================================ the 20 x 20 capsule pairs: thread (hand, bone k) walks the other hand's bones in order
        if (run_col && lt >= 64 && lt < 84) {
#pragma clang fp contract(off)
            const int k = lt - 64;
            float acc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, go[3] = {0.f, 0.f, 0.f}, rowe = 0.f, rowm = 0.f;
            int nact = 0, nodir_any = 0;
            for (int m = 0; m < 20; ++m) {
                const int i = hand ? m : k, j = hand ? k : m;           // left bone i, right bone j
                const int ia = kParent[i], ib = kChild[i], jc = kParent[j], jd = kChild[j];
                const float A[3] = {s_x[0][3 * ia], s_x[0][3 * ia + 1], s_x[0][3 * ia + 2]}, B[3] = {s_x[0][3 * ib], s_x[0][3 * ib + 1], s_x[0][3 * ib + 2]};
                const float C[3] = {s_x[1][3 * jc], s_x[1][3 * jc + 1], s_x[1][3 * jc + 2]}, D[3] = {s_x[1][3 * jd], s_x[1][3 * jd + 1], s_x[1][3 * jd + 2]};
                float h, gA[3], gB[3], gC[3], gD[3];
                bool active, nodir;
                fit::capsule_pair(A, B, C, D, s_rad[0][i] + s_rad[1][j], args.k_col, h, active, nodir, gA, gB, gC, gD);
                nodir_any |= nodir;
                if (h > 0.f) { rowe = rowe + h * h; rowm = fmaxf(rowm, h); }
                if (active) {
                    ++nact;
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        acc[c] = acc[c] + (hand ? gC[c] : gA[c]);
                        acc[3 + c] = acc[3 + c] + (hand ? gD[c] : gB[c]);
                        go[c] = go[c] + (gC[c] + gD[c]);
                    }
                }
            }
#pragma unroll
            for (int c = 0; c < 6; ++c) s_bone[hand][k][c] = acc[c];
            s_bact[hand][k] = nact;
            if (hand == 0) {
                s_rowe[k] = rowe; s_rowm[k] = rowm; s_nodir[k] = nodir_any;
                s_rowgo[k][0] = go[0]; s_rowgo[k][1] = go[1]; s_rowgo[k][2] = go[2];
            }
        }
        __syncthreads();
        if (want_mse && lt < 3) {
            const float mse = fit::mean_sq(s_sum, use_v, lt);
            if (it == 0) s_mse[lt] = mse;
            if (last) s_mse[3 + lt] = mse;
        }
        int nodir_now = 0;
        if (run_col) {
#pragma clang fp contract(off)
            // the bones' sums into the joints' cotangents and into the hand's sum of cotangents, bone-index order; a bone without an active pair is skipped
            if (grad_col && !last && lt < 21) {
                float g[3] = {0.f, 0.f, 0.f};
                int any = 0;
                for (int k = 0; k < 20; ++k) {
                    if (!s_bact[hand][k]) continue;
                    if (kParent[k] == lt) { any = 1; g[0] = g[0] + s_bone[hand][k][0]; g[1] = g[1] + s_bone[hand][k][1]; g[2] = g[2] + s_bone[hand][k][2]; }
                    if (kChild[k] == lt) { any = 1; g[0] = g[0] + s_bone[hand][k][3]; g[1] = g[1] + s_bone[hand][k][4]; g[2] = g[2] + s_bone[hand][k][5]; }
                }
                if (any) { G.gj[3 * lt] = G.gj[3 * lt] + g[0]; G.gj[3 * lt + 1] = G.gj[3 * lt + 1] + g[1]; G.gj[3 * lt + 2] = G.gj[3 * lt + 2] + g[2]; }
            }
            if (grad_col && !last && lt >= 32 && lt < 35) {
                const int c = lt - 32;
                float g = 0.f;
                int any = 0;
                for (int k = 0; k < 20; ++k)
                    if (s_bact[hand][k]) { any = 1; g = g + (s_bone[hand][k][c] + s_bone[hand][k][3 + c]); }
                if (any) s_sum[c] = s_sum[c] + g;
            }
            if (tid >= 64 && tid < 67) {                                 // g_o of the collision term (0 where no pair is active)
                const int c = tid - 64;
                float g = 0.f;
                for (int k = 0; k < 20; ++k)
                    if (s_bact[0][k]) g = g + s_rowgo[k][c];
                s_go[c] = grad_col ? g : 0.f;
            }
            if (tid == 96) {
                float e = 0.f, mx = 0.f;
                for (int k = 0; k < 20; ++k) { e = e + s_rowe[k]; mx = fmaxf(mx, s_rowm[k]); }
                e = e / 400.f;
                if (it == 0) { s_col[0] = e; s_col[1] = mx; }
                if (last) { s_col[2] = e; s_col[3] = mx; }
            }
            for (int k = 0; k < 20; ++k) nodir_now |= s_nodir[k];     // every thread reads the same 20 flags
        }
        if (nodir_now) pstatus |= 8;
        if (last) break;
        __syncthreads();                                                  // the gather wrote gj and s_sum, which centre_bwd reads

        // ================================================================ backward (mano_device.h, layers 3 and 4), the gradient into s_g
        DIR_MANO_BACKWARD_SCHEDULE(dir::wave_sum_dpp, G, L, T, side, center, root_palm, s_sum, s_v, s_gv, s_gvp, lt);
        rodrigues_bwd(G, L, s_full, lt);
        if (lt == 64) robust6d_bwd(s_pose, G.groot, s_g);
        fit::gradient_tail(G, T, s_gvp, s_sum, s_g, lt);
        __syncthreads();
        if (lt < 45) s_g[6 + lt] = pca_bwd(G, T, lt);
        __syncthreads();

        // ================================================================ the priors' gradients and one Adam step per hand; the fifth group, o
        float p_new = 0.f, m_new = 0.f, v_new = 0.f;
        int bad = 0, bad_step_o = 0;
        const float pb1n = pb1 * args.r.b1, pb2n = pb2 * args.r.b2, po1n = po1 * args.r.b1, po2n = po2 * args.r.b2;
        if (lt < 64 && alive) {
            const float p = s_p[lt];
            const float g = fit::prior_gradient(lt, s_g[lt], p, s_anchor[lt], args.r.k_pca, args.r.k_beta, args.r.k_init);
            p_new = p; m_new = s_m[lt]; v_new = s_vv[lt];
            bad = !fit::adam(g, args.r.lr[fit::group_of(lt)], args.r.b1, args.r.b2, args.r.eps, pb1n, pb2n, p_new, m_new, v_new);
        }
        if (tid >= 64 && tid < 67 && o_alive) {
#pragma clang fp contract(off)
            const int c = tid - 64;
            const float o = s_o[c];
            float g = grad_col ? s_go[c] : 0.f;
            if (use_ot) g = g + (args.k_off * c_o) * (o - s_ot[c]);
            g = g + args.k_oi * (o - s_oa[c]);
            p_new = o; m_new = s_om[c]; v_new = s_ov[c];
            bad_step_o = !fit::adam(g, args.lr_o, args.r.b1, args.r.b2, args.r.eps, po1n, po2n, p_new, m_new, v_new);
        }
        const bool bad_l = __syncthreads_or(bad && hand == 0) != 0, bad_r = __syncthreads_or(bad && hand == 1) != 0;
        const bool bad_o_step = __syncthreads_or(bad_step_o) != 0;
        if (alive) {
            if (hand ? bad_r : bad_l) { status |= 4; alive = false; }   // the step is not taken: the hand stays at its last finite iterate, as an obstacle
            else {
                if (lt < 64) { s_p[lt] = p_new; s_m[lt] = m_new; s_vv[lt] = v_new; }
                pb1 = pb1n; pb2 = pb2n; ++t_step;
            }
        }
        if (other_alive && (hand ? bad_l : bad_r)) other_alive = false;
        if (o_alive) {
            if (bad_o_step) { pstatus |= 4; o_alive = false; }
            else {
                if (tid >= 64 && tid < 67) { s_o[tid - 64] = p_new; s_om[tid - 64] = m_new; s_ov[tid - 64] = v_new; }
                po1 = po1n; po2 = po2n; ++t_o;
            }
        }
        __syncthreads();
    }

    // ================================================================ outputs at the final iterate (the forward above ran at it)
    __syncthreads();
    fit::write_outputs(a, b, L, s_vert, s_cam, p0_bad, lt);
    fit::store_row(a, b, pass, s_p0, s_p, s_m, s_vv, lt);
    if (lt == 64) {
        if (a.state && !pass) fit::store_clock(a.state, b, pb1, pb2, t_step);
        if (a.status) a.status[b] = status | (p0_bad ? 0 : s_flag2[hand]);
    }
    if (a.mse && lt >= 128 && lt < 134) a.mse[b * 6 + lt - 128] = p0_bad ? 0.f : s_mse[lt - 128];
    // the pair's
    if (tid >= 192 && tid < 195) {
        const int c = tid - 192;
        pa.offset_out[b * 3 + c] = coupled ? s_o[c] : s_o0[c];
        if (pa.o_state && coupled) { pa.o_state[b * OST + c] = s_om[c]; pa.o_state[b * OST + 3 + c] = s_ov[c]; }
    }
    if (tid == 195) {
        if (pa.o_state && coupled) {
            pa.o_state[b * OST + 6] = po1; pa.o_state[b * OST + 7] = po2; pa.o_state[b * OST + 8] = __int_as_float(t_o);
            pa.o_state[b * OST + 9] = 0.f; pa.o_state[b * OST + 10] = 0.f; pa.o_state[b * OST + 11] = 0.f;
        }
        if (pa.pair_status) pa.pair_status[b] = pstatus;
    }
    if (pa.col && tid >= 196 && tid < 200) pa.col[b * 4 + tid - 196] = coupled ? s_col[tid - 196] : 0.f;
}

}  // namespace

extern "C" int dir_mano_fit_pair(const dir_mano_tables* tables_host, const dir_mano_fit_hand* hands_host, const dir_mano_fit_opts* opts_host,
                                 const dir_mano_fit_pair_args* pair_host, const dir_mano_fit_pair_opts* pair_opts_host, int B, void* stream) {
    using namespace dir;
    if (B == 0) return DIR_OK;
    DIR_REQUIRE(B > 0 && tables_host && hands_host && opts_host && pair_host && pair_opts_host, "dir_mano_fit_pair: bad arguments");
    const dir_mano_fit_pair_opts& q = *pair_opts_host;
    PairArgs a;
    if (int rc = mano::fit::check_opts(*opts_host, {q.w_col, q.w_off, q.w_off_init, q.lr_o}, "dir_mano_fit_pair", a.r)) return rc;
    const dir_mano_fit_pair_args& p = *pair_host;
    DIR_REQUIRE(p.o0 && p.offset_out && p.radii[0] && p.radii[1], "dir_mano_fit_pair: null pointer (o0 / offset_out / radii)");
    DIR_REQUIRE(!p.o_conf || p.o_target, "dir_mano_fit_pair: o_conf without o_target");
    for (int h = 0; h < 2; ++h) {
        const dir_mano_tables& t = tables_host[h];
        if (int rc = mano::check_mano_tables(t, "dir_mano_fit_pair")) return rc;
        if (int rc = mano::fit::check_hand(hands_host[h], "dir_mano_fit_pair")) return rc;
        a.t[h] = t;
        a.h[h] = hands_host[h];
    }
    a.p = p;
    a.k_col = (float)(2.0 * q.w_col / 400.0); a.k_off = 2.f * q.w_off; a.k_oi = 2.f * q.w_off_init; a.lr_o = q.lr_o;
    DIR_LAUNCH(mano_fit_pair_kernel, dim3(B), dim3(PT), 0, (hipStream_t)stream, a);
    return check_launch("dir_mano_fit_pair");
}
