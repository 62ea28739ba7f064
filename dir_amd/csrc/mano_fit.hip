// dir_mano_fit: MANO parameters fitted to meshes, 3-D joints and 2-D keypoints -- dir_mano_forward run the other way.  Per (sample, hand)
// the 64-vector p (pose 51 = 6D root | 45 PCA, betas 10, cam 3) is moved by `iters` Adam steps down the residual E(p) of
// include/dir_hip.h ("MANO fitting"); the rule, the order of every operation and the status bits are written out there.
//
// One 256-thread workgroup per (sample, hand), as mano_backward_kernel, and the iteration loop is INSIDE the kernel: the parameters, the
// Adam state, the posed and skinned vertices and their cotangents stay in LDS (46 KB) from the first iteration to the last; per
// iteration only the tables (L2 resident, shared by every workgroup) and the targets (9.3 KB per hand) are read from memory.  Composed from
// the existing launches one iteration is a forward, a few ATen residual operations, a backward and an optimiser step (measured: DESIGN.md, "MANO fitting").
//
// The forward and the backward are mano_device.h's phases, the ones mano.hip and mano_bwd.hip run (the outputs at iters = 0 are
// dir_mano_forward's bits); unlike dir_mano_backward_pair this entry point accepts the root_palm wrist.  The residuals, the mean squared
// errors and the Adam step are mano_fit_device.h's, shared with the sequence fit (mano_fit_seq.hip).
// fp32 throughout, every reduction in a fixed order, no atomics, no scratch buffer: a row gives the same bits in any slot of any batch and
// in either hand slot.
#include "mano_fit_device.h"

namespace {

using namespace dir::mano;
using dir::finite;

constexpr int ST = DIR_MANO_FIT_STATE;

struct FitArgs {
    dir_mano_tables t[2];
    dir_mano_fit_hand h[2];
    float kv, kj, kuv;                   // 2 w_v / 778, 2 w_j / 21, 2 w_uv / 21: formed in double on the host, rounded once
    float k_pca, k_beta, k_init;         // 2 w_pca, 2 w_beta, 2 w_init
    float lr[4], b1, b2, eps;
    int iters;
};

__global__ __launch_bounds__(BT) void mano_fit_kernel(FitArgs args) {
    const dir_mano_tables& T = args.t[blockIdx.y];
    const dir_mano_fit_hand& a = args.h[blockIdx.y];
    const int side = T.side, center = T.center_idx, root_palm = T.root_palm;       // read once, here (mano_device.h, layer 2)
    __shared__ float s_v[NV3P];          // v_posed
    __shared__ float s_vert[NV3P];       // skinned vertices (before centring)
    __shared__ float s_gv[NV3P];         // g of the skinned vertices
    __shared__ float s_gvp[NV3P];        // g of v_posed (= g of v_shaped)
    __shared__ float s_p[64], s_p0[64], s_anchor[64], s_m[64], s_vv[64], s_g[64];      // iterate, start, prior centre, Adam moments, gradient
    __shared__ float s_full[45];
    DIR_MANO_LDS(L, s);
    DIR_MANO_BWD_LDS(G, s);
    __shared__ float s_red[4][11], s_sum[11], s_mse[6];
    __shared__ int s_flag;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t b = blockIdx.x;
    const float* s_pose = s_p;
    const float* s_beta = s_p + 51;
    const float* s_cam = s_p + 61;

    // ================================================================ start: the row, its state, and the pass-through test (status bit 1)
    float pb1 = 1.f, pb2 = 1.f;          // b1^t, b2^t as running fp32 products (every thread carries the same values)
    int t_step = 0;
    if (a.state) {
        t_step = __float_as_int(a.state[b * ST + 130]);
        if (t_step > 0) { pb1 = a.state[b * ST + 128]; pb2 = a.state[b * ST + 129]; }
    }
    int bad_p = 0, bad_t = 0;
    if (tid < 64) {
        const float x = a.p0[b * 64 + tid];
        const float an = a.anchor ? a.anchor[b * 64 + tid] : x;
        s_p0[tid] = x; s_p[tid] = x; s_anchor[tid] = an;
        s_m[tid] = a.state ? a.state[b * ST + tid] : 0.f;
        s_vv[tid] = a.state ? a.state[b * ST + 64 + tid] : 0.f;
        bad_p = !finite(x) || !finite(an);
    }
    if (a.verts_t)
        for (int i = tid; i < NV3; i += BT) bad_t |= !finite(a.verts_t[b * NV3 + i]);
    if (tid < 21) {
        if (a.joints_t) {
            const float c = a.joints_conf ? a.joints_conf[b * 21 + tid] : 1.f;
            if (c > 0.f) {
                const float* t = a.joints_t + (b * 21 + tid) * 3;
                bad_t |= !finite(c) || !finite(t[0]) || !finite(t[1]) || !finite(t[2]);
            }
        }
        if (a.uv_t) {
            const float d = a.uv_conf ? a.uv_conf[b * 21 + tid] : 1.f;
            if (d > 0.f) {
                const float* t = a.uv_t + (b * 21 + tid) * 2;
                bad_t |= !finite(d) || !finite(t[0]) || !finite(t[1]);
            }
        }
    }
    const bool p0_bad = __syncthreads_or(bad_p) != 0;
    const bool pass = __syncthreads_or(bad_t) != 0 || p0_bad;           // the row passes through: no step, no target enters the arithmetic
    const bool use_v = a.verts_t && !pass, use_j = a.joints_t && !pass, use_uv = a.uv_t && !pass;
    int n_it = pass ? 0 : args.iters;
    int status = pass ? 2 : 0;

    for (int it = 0;; ++it) {
        // ================================================================ forward at s_p (mano_device.h, layer 2)
        if (tid < 45) s_full[tid] = pca_axis_angle(T, s_pose + 6, tid);
        shape_blend(T, s_beta, s_v, tid);
        if (tid == 64) { int reflect; robust6d(s_pose, L.root, reflect); s_flag = reflect; }
        __syncthreads();
        joint_rotations(L, s_full, tid);
        joint_regression(L, T, s_beta, tid);
        __syncthreads();
        pose_blend(L, T, s_v, tid);
        chain(L, tid);
        __syncthreads();
        a_primes(L, tid);
        __syncthreads();
        skinning(L, T, s_v, s_vert, tid);
        __syncthreads();
        joints(L, side, root_palm, s_vert, tid);
        __syncthreads();
        centre(L, center, tid);
        __syncthreads();

        // ================================================================ residuals: the cotangents gV, gJ, gU; the mean squared residuals at p0 and at the end
        const bool last = it >= n_it, want_mse = it == 0 || last;
        float red[11] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};     // sum g.x, g.y, g.z | g s | g tx, g ty | sq V | sq J, n J | sq U, n U
        fit::residuals(a, b, L, G, s_vert, s_gv, s_cam, use_v, use_j, use_uv, args.kv, args.kj, args.kuv, tid, red);
        fit::residual_partials(red, want_mse, s_red, lane, wave);
        if (tid < 48) { G.gAt[tid] = 0.f; }
        __syncthreads();
        if (tid < 11) s_sum[tid] = s_red[0][tid] + s_red[1][tid] + s_red[2][tid] + s_red[3][tid];
        __syncthreads();
        if (want_mse && tid < 3) {
            const float mse = fit::mean_sq(s_sum, use_v, tid);
            if (it == 0) s_mse[tid] = mse;
            if (last) s_mse[3 + tid] = mse;
        }
        if (last) break;

        // ================================================================ backward (mano_device.h, layer 3), the gradient into s_g
        centre_bwd(G, center, s_sum, tid);
        __syncthreads();
        joints_bwd(G, side, root_palm, s_gv, tid);
        __syncthreads();
        skinning_bwd(L, T, s_gv, s_gvp, tid);
        a_primes_grad(G, T, s_gv, s_v, tid);
        __syncthreads();
        a_primes_bwd(G, L, tid);
        __syncthreads();
        chain_bwd(G, L, tid);
        __syncthreads();
        chain_root_bwd(G, tid);
        __syncthreads();
        root_split_bwd(G, tid);
        pose_blend_bwd<dir::wave_sum_dpp>(L, T, s_gvp, tid);          // (L.pm re-used: the next forward writes it again)
        __syncthreads();
        rodrigues_bwd(G, L, s_full, tid);
        if (tid == 64) robust6d_bwd(s_pose, G.groot, s_g);
        for (int k = wave; k < 10; k += BT / 64) {
            const float acc = shape_blend_bwd<dir::wave_sum_dpp>(G, T, s_gvp, k, lane);
            if (lane == 0) s_g[51 + k] = acc;
        }
        if (tid >= 128 && tid < 131) s_g[61 + tid - 128] = s_sum[3 + tid - 128];
        __syncthreads();
        if (tid < 45) s_g[6 + tid] = pca_bwd(G, T, tid);
        __syncthreads();

        // ================================================================ the priors' gradients and one Adam step (include/dir_hip.h gives this order)
        float p_new = 0.f, m_new = 0.f, v_new = 0.f;
        int bad = 0;
        const float pb1n = pb1 * args.b1, pb2n = pb2 * args.b2;
        if (tid < 64) {
            const float p = s_p[tid];
            const float g = fit::prior_gradient(tid, s_g[tid], p, s_anchor[tid], args.k_pca, args.k_beta, args.k_init);
            p_new = p; m_new = s_m[tid]; v_new = s_vv[tid];
            bad = !fit::adam(g, args.lr[fit::group_of(tid)], args.b1, args.b2, args.eps, pb1n, pb2n, p_new, m_new, v_new);
        }
        if (__syncthreads_or(bad)) {          // the step is not taken: the last finite iterate and its state stay, and the loop ends
            status |= 4;
            n_it = it + 1;
        } else {
            if (tid < 64) { s_p[tid] = p_new; s_m[tid] = m_new; s_vv[tid] = v_new; }
            pb1 = pb1n; pb2 = pb2n; ++t_step;
        }
        __syncthreads();
    }

    // ================================================================ outputs at the final iterate (the forward above ran at it)
    __syncthreads();
    if (a.verts)
        for (int i = tid; i < NV3; i += BT) a.verts[b * NV3 + i] = p0_bad ? 0.f : s_vert[i] - L.c[i % 3];
    if (a.joints && tid < 63) a.joints[b * 63 + tid] = p0_bad ? 0.f : L.jtr[tid] - L.c[tid % 3];
    if (a.joint_uv && tid >= 64 && tid < 64 + 42) {
        const int i = tid - 64, j = i >> 1, c = i & 1;
        a.joint_uv[b * 42 + i] = p0_bad ? 0.f : s_cam[0] * (L.jtr[3 * j + c] - L.c[c]) + (c ? s_cam[2] : s_cam[1]);
    }
    if (tid < 64) {
        a.p_out[b * 64 + tid] = pass ? s_p0[tid] : s_p[tid];
        if (a.state && !pass) { a.state[b * ST + tid] = s_m[tid]; a.state[b * ST + 64 + tid] = s_vv[tid]; }
    }
    if (tid == 64) {
        if (a.state && !pass) {
            a.state[b * ST + 128] = pb1; a.state[b * ST + 129] = pb2;
            a.state[b * ST + 130] = __int_as_float(t_step); a.state[b * ST + 131] = 0.f;
        }
        if (a.status) a.status[b] = status | (p0_bad ? 0 : s_flag);
    }
    if (a.mse && tid >= 128 && tid < 134) a.mse[b * 6 + tid - 128] = p0_bad ? 0.f : s_mse[tid - 128];
}

}  // namespace

extern "C" int dir_mano_fit(const dir_mano_tables* tables_host, const dir_mano_fit_hand* hands_host, const dir_mano_fit_opts* opts_host,
                            int hands, int B, void* stream) {
    using namespace dir;
    if (B == 0) return DIR_OK;
    DIR_REQUIRE(B > 0 && (hands == 1 || hands == 2) && tables_host && hands_host && opts_host, "dir_mano_fit: bad arguments");
    const dir_mano_fit_opts& o = *opts_host;
    DIR_REQUIRE(o.iters >= 0, "dir_mano_fit: iters must be >= 0");
    for (float w : {o.w_verts, o.w_joints, o.w_uv, o.w_pca, o.w_beta, o.w_init, o.lr[0], o.lr[1], o.lr[2], o.lr[3]})
        DIR_REQUIRE(w >= 0.f && w <= 3.4e38f, "dir_mano_fit: weights and learning rates must be finite and >= 0");
    DIR_REQUIRE(o.b1 >= 0.f && o.b1 < 1.f && o.b2 >= 0.f && o.b2 < 1.f && o.eps > 0.f, "dir_mano_fit: need 0 <= b1, b2 < 1 and eps > 0");
    FitArgs a;
    for (int h = 0; h < hands; ++h) {
        const dir_mano_tables& t = tables_host[h];
        if (int rc = mano::check_mano_tables(t, "dir_mano_fit")) return rc;
        const dir_mano_fit_hand& f = hands_host[h];
        DIR_REQUIRE(f.p0 && f.p_out, "dir_mano_fit: null pointer (p0 / p_out)");
        DIR_REQUIRE((!f.joints_conf || f.joints_t) && (!f.uv_conf || f.uv_t), "dir_mano_fit: confidences without their target");
        a.t[h] = t;
        a.h[h] = f;
    }
    if (hands == 1) { a.t[1] = a.t[0]; a.h[1] = a.h[0]; }
    a.kv = (float)(2.0 * o.w_verts / 778.0); a.kj = (float)(2.0 * o.w_joints / 21.0); a.kuv = (float)(2.0 * o.w_uv / 21.0);
    a.k_pca = 2.f * o.w_pca; a.k_beta = 2.f * o.w_beta; a.k_init = 2.f * o.w_init;
    for (int g = 0; g < 4; ++g) a.lr[g] = o.lr[g];
    a.b1 = o.b1; a.b2 = o.b2; a.eps = o.eps; a.iters = o.iters;
    DIR_LAUNCH(mano_fit_kernel, dim3(B, hands), dim3(BT), 0, (hipStream_t)stream, a);
    return check_launch("dir_mano_fit");
}
