// dir_mano_fit: MANO parameters fitted to meshes, 3-D joints and 2-D keypoints -- dir_mano_forward run the other way.  Per (sample, hand)
// the 64-vector p (pose 51 = 6D root | 45 PCA, betas 10, cam 3) is moved by `iters` Adam steps down the residual E(p) of
// include/dir_hip.h ("MANO fitting"); the rule, the order of every operation and the status bits are written out there.
//
// One 256-thread workgroup per (sample, hand), as mano_backward_kernel, and the iteration loop is INSIDE the kernel: the parameters, the
// Adam state, the posed and skinned vertices and their cotangents stay in LDS (46 KB) from the first iteration to the last; per
// iteration only the tables (L2 resident, shared by every workgroup) and the targets (9.3 KB per hand) are read from memory.  Composed from
// the existing launches one iteration is a forward, a few ATen residual operations, a backward and an optimiser step (measured: DESIGN.md, "MANO fitting").
//
// The forward and the backward are mano_device.h's two schedules over its phases, the ones mano_bwd.hip runs (the outputs at iters = 0 are
// dir_mano_forward's bits); unlike dir_mano_backward_pair this entry point accepts the root_palm wrist.  The checks of the options, the target
// scan, the row and the Adam clock, the residuals, the mean squared errors, the gradient's tail, the Adam step and the output block are
// mano_fit_device.h's, shared with the sequence fit (mano_fit_seq.hip) and the pair fit (mano_fit_pair.hip); what stands here is the loop.
// fp32 throughout, every reduction in a fixed order, no atomics, no scratch buffer: a row gives the same bits in any slot of any batch and
// in either hand slot.
#include "mano_fit_device.h"

namespace {

using namespace dir::mano;

struct FitArgs {
    dir_mano_tables t[2];
    dir_mano_fit_hand h[2];
    fit::Rule r;
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
    float pb1, pb2;                      // b1^t, b2^t
    int t_step;
    fit::load_clock(a.state, b, pb1, pb2, t_step);
    const int bad_p = fit::load_row(a, b, s_p0, s_p, s_anchor, s_m, s_vv, tid);
    const int bad_t = fit::targets_nonfinite(a, b, tid);
    const bool p0_bad = __syncthreads_or(bad_p) != 0;
    const bool pass = __syncthreads_or(bad_t) != 0 || p0_bad;           // the row passes through: no step, no target enters the arithmetic
    const bool use_v = a.verts_t && !pass, use_j = a.joints_t && !pass, use_uv = a.uv_t && !pass;
    int n_it = pass ? 0 : args.r.iters;
    int status = pass ? 2 : 0;

    for (int it = 0;; ++it) {
        // ================================================================ forward at s_p (mano_device.h, layers 2 and 4)
        if (tid < 45) s_full[tid] = pca_axis_angle(T, s_pose + 6, tid);
        shape_blend(T, s_beta, s_v, tid);
        if (tid == 64) { int reflect; robust6d(s_pose, L.root, reflect); s_flag = reflect; }
        __syncthreads();
        forward_schedule(L, T, side, center, root_palm, s_full, s_beta, s_v, s_vert, tid);
        __syncthreads();

        // ================================================================ residuals: the cotangents gV, gJ, gU; the mean squared residuals at p0 and at the end
        const bool last = it >= n_it, want_mse = it == 0 || last;
        float red[11] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};     // sum g.x, g.y, g.z | g s | g tx, g ty | sq V | sq J, n J | sq U, n U
        fit::residuals(a, b, L, G, s_vert, s_gv, s_cam, use_v, use_j, use_uv, args.r.kv, args.r.kj, args.r.kuv, tid, red);
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

        // ================================================================ backward (mano_device.h, layers 3 and 4), the gradient into s_g
        DIR_MANO_BACKWARD_SCHEDULE(dir::wave_sum_dpp, G, L, T, side, center, root_palm, s_sum, s_v, s_gv, s_gvp, tid);      // (L.pm re-used: the next forward writes it again)
        rodrigues_bwd(G, L, s_full, tid);
        if (tid == 64) robust6d_bwd(s_pose, G.groot, s_g);
        fit::gradient_tail(G, T, s_gvp, s_sum, s_g, tid);
        __syncthreads();
        if (tid < 45) s_g[6 + tid] = pca_bwd(G, T, tid);
        __syncthreads();

        // ================================================================ the priors' gradients and one Adam step (include/dir_hip.h gives this order)
        float p_new = 0.f, m_new = 0.f, v_new = 0.f;
        int bad = 0;
        const float pb1n = pb1 * args.r.b1, pb2n = pb2 * args.r.b2;
        if (tid < 64) {
            const float p = s_p[tid];
            const float g = fit::prior_gradient(tid, s_g[tid], p, s_anchor[tid], args.r.k_pca, args.r.k_beta, args.r.k_init);
            p_new = p; m_new = s_m[tid]; v_new = s_vv[tid];
            bad = !fit::adam(g, args.r.lr[fit::group_of(tid)], args.r.b1, args.r.b2, args.r.eps, pb1n, pb2n, p_new, m_new, v_new);
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
    fit::write_outputs(a, b, L, s_vert, s_cam, p0_bad, tid);
    fit::store_row(a, b, pass, s_p0, s_p, s_m, s_vv, tid);
    if (tid == 64) {
        if (a.state && !pass) fit::store_clock(a.state, b, pb1, pb2, t_step);
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
    FitArgs a;
    if (int rc = mano::fit::check_opts(*opts_host, {}, "dir_mano_fit", a.r)) return rc;
    for (int h = 0; h < hands; ++h) {
        const dir_mano_tables& t = tables_host[h];
        if (int rc = mano::check_mano_tables(t, "dir_mano_fit")) return rc;
        if (int rc = mano::fit::check_hand(hands_host[h], "dir_mano_fit")) return rc;
        a.t[h] = t;
        a.h[h] = hands_host[h];
    }
    if (hands == 1) { a.t[1] = a.t[0]; a.h[1] = a.h[0]; }
    DIR_LAUNCH(mano_fit_kernel, dim3(B, hands), dim3(BT), 0, (hipStream_t)stream, a);
    return check_launch("dir_mano_fit");
}
