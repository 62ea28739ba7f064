// Backward of the fused MANO layer + weak-perspective projection (dir_mano_forward): the gradient of
//   <g_verts, verts> + <g_joints, joints> + <g_joint_uv, joint_uv> + <g_mesh_uv, mesh_uv>
// w.r.t. the 64-vector a regressor predicts per hand (pose 51 = 6D root | 45 PCA, betas 10, cam 3; models/dir.py:352-363) --
// what torch autograd computes through manopth/manopth/manolayer.py:110-270 (+ rodrigues_layer.py:15-54, rot6d.py:26-60,
// tensutils.py:6-42) and utils/utils.py:47-63 in the reference's training step (train.py:66-70).  First link of the backward
// pass behind dir_stage_losses_backward.
//
// One 256-thread workgroup per (sample, hand).  The forward is recomputed in LDS (pose maths, chain, posed and skinned vertices:
// cheaper than round-tripping 30 KB of intermediates per (sample, hand) through HBM) by mano_device.h's forward schedule, then reversed
// stage by stage by its backward schedule (the three fit kernels run the same two); the projection and the cotangents are this kernel's own:
//   projection / centring -> joint routing (chain joints, fingertip vertices) -> skinning (g v_posed per vertex; g A'_k as 192
//   reductions over the 778 vertices) -> A' -> A -> kinematic chain (one thread per finger, root partials combined afterwards)
//   -> pose blend shapes (135 wave-level dot products over the k-major table) -> Rodrigues-via-quaternion and robust-6D chain
//   rules -> PCA and shape blend (10 wave-level dot products + the folded joint regressor).
// Reductions run in a fixed order (no atomics): results are deterministic.  fp32 throughout, like the forward.
#include "mano_device.h"

namespace {

using namespace dir::mano;

struct ManoBwdHand {
    dir_mano_tables t;
    const float* pose; int pose_stride;
    const float* betas; int betas_stride;
    const float* cam; int cam_stride;
    const float* g_verts; const float* g_joints; const float* g_joint_uv; const float* g_mesh_uv;
    float* g_pose; int g_pose_stride;
    float* g_betas; int g_betas_stride;
    float* g_cam; int g_cam_stride;
};
struct ManoBwdArgs { ManoBwdHand h[2]; };

__global__ __launch_bounds__(BT) void mano_backward_kernel(ManoBwdArgs args) {
    const ManoBwdHand& a = args.h[blockIdx.y];
    const dir_mano_tables& T = a.t;
    const int side = T.side, center = T.center_idx, root_palm = T.root_palm;       // read once, here (mano_device.h, layer 2)
    __shared__ float s_v[NV3P];          // v_posed
    __shared__ float s_vert[NV3P];       // skinned vertices (before centring)
    __shared__ float s_gv[NV3P];         // g of the skinned vertices
    __shared__ float s_gvp[NV3P];        // g of v_posed (= g of v_shaped)
    __shared__ float s_pose[51], s_beta[10], s_cam[3], s_full[45];
    DIR_MANO_LDS(L, s);
    DIR_MANO_BWD_LDS(G, s);
    __shared__ float s_red[4][6], s_sum[6];

    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    // ================================================================ forward (mano_device.h, layers 2 and 4)
    if (tid < 51) s_pose[tid] = a.pose[(size_t)b * a.pose_stride + tid];
    if (tid >= 64 && tid < 74) s_beta[tid - 64] = a.betas[(size_t)b * a.betas_stride + tid - 64];
    if (tid >= 128 && tid < 131) s_cam[tid - 128] = a.cam ? a.cam[(size_t)b * a.cam_stride + tid - 128] : 0.f;
    __syncthreads();
    if (tid < 45) s_full[tid] = pca_axis_angle(T, s_pose + 6, tid);
    shape_blend(T, s_beta, s_v, tid);
    if (tid == 64) { int reflect; robust6d(s_pose, L.root, reflect); }
    __syncthreads();
    forward_schedule(L, T, side, center, root_palm, s_full, s_beta, s_v, s_vert, tid);
    __syncthreads();

    // ================================================================ backward
    // ---- projection (uv = s (p - c).xy + t) and centring: g of every position, sum of them (-> g c), g s, g t
    const float sc = s_cam[0];
    float red[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};       // sum g.x, g.y, g.z | g s | g tx, g ty
    for (int v = tid; v < NV; v += BT) {
        float gx = 0.f, gy = 0.f, gz = 0.f;
        if (a.g_verts) { const float* g = a.g_verts + ((size_t)b * NV + v) * 3; gx = g[0]; gy = g[1]; gz = g[2]; }
        if (a.g_mesh_uv && a.cam) {
            const float* g = a.g_mesh_uv + ((size_t)b * NV + v) * 2;
            red[3] += g[0] * (s_vert[3 * v] - L.c[0]) + g[1] * (s_vert[3 * v + 1] - L.c[1]);
            red[4] += g[0]; red[5] += g[1];
            gx = fmaf(sc, g[0], gx); gy = fmaf(sc, g[1], gy);
        }
        s_gv[3 * v] = gx; s_gv[3 * v + 1] = gy; s_gv[3 * v + 2] = gz;
        red[0] += gx; red[1] += gy; red[2] += gz;
    }
    if (tid < 21) {
        float gx = 0.f, gy = 0.f, gz = 0.f;
        if (a.g_joints) { const float* g = a.g_joints + ((size_t)b * 21 + tid) * 3; gx = g[0]; gy = g[1]; gz = g[2]; }
        if (a.g_joint_uv && a.cam) {
            const float* g = a.g_joint_uv + ((size_t)b * 21 + tid) * 2;
            red[3] += g[0] * (L.jtr[3 * tid] - L.c[0]) + g[1] * (L.jtr[3 * tid + 1] - L.c[1]);
            red[4] += g[0]; red[5] += g[1];
            gx = fmaf(sc, g[0], gx); gy = fmaf(sc, g[1], gy);
        }
        G.gj[3 * tid] = gx; G.gj[3 * tid + 1] = gy; G.gj[3 * tid + 2] = gz;
        red[0] += gx; red[1] += gy; red[2] += gz;
    }
#pragma unroll
    for (int e = 0; e < 6; ++e) { const float s = dir::wave_sum(red[e]); if (lane == 0) s_red[wave][e] = s; }
    if (tid < 48) { G.gAt[tid] = 0.f; }
    __syncthreads();
    if (tid < 6) s_sum[tid] = s_red[0][tid] + s_red[1][tid] + s_red[2][tid] + s_red[3][tid];
    __syncthreads();
    // ---- the layer's backward (mano_device.h, layers 3 and 4)
    DIR_MANO_BACKWARD_SCHEDULE(dir::wave_sum, G, L, T, side, center, root_palm, s_sum, s_v, s_gv, s_gvp, tid);
    rodrigues_bwd(G, L, s_full, tid);
    if (tid == 64 && a.g_pose) robust6d_bwd(s_pose, G.groot, a.g_pose + (size_t)b * a.g_pose_stride);
    for (int k = wave; k < 10; k += BT / 64) {
        const float acc = shape_blend_bwd<dir::wave_sum>(G, T, s_gvp, k, lane);
        if (lane == 0 && a.g_betas) a.g_betas[(size_t)b * a.g_betas_stride + k] = acc;
    }
    __syncthreads();
    if (tid < 45 && a.g_pose) a.g_pose[(size_t)b * a.g_pose_stride + 6 + tid] = pca_bwd(G, T, tid);
    if (tid >= 64 && tid < 67 && a.g_cam) a.g_cam[(size_t)b * a.g_cam_stride + tid - 64] = a.cam ? s_sum[3 + tid - 64] : 0.f;
}

}  // namespace

extern "C" int dir_mano_backward_pair(const dir_mano_tables* tables_lr, const float* const* pose_lr, int pose_stride,
                                      const float* const* betas_lr, int betas_stride, const float* const* cam_lr, int cam_stride,
                                      const float* const* g_verts_lr, const float* const* g_joints_lr, const float* const* g_joint_uv_lr,
                                      const float* const* g_mesh_uv_lr, float* const* g_pose_lr, int g_pose_stride, float* const* g_betas_lr,
                                      int g_betas_stride, float* const* g_cam_lr, int g_cam_stride, int hands, int B, void* stream) {
    using namespace dir;
    if (B == 0) return DIR_OK;
    DIR_REQUIRE(B > 0 && (hands == 1 || hands == 2) && tables_lr && pose_lr && betas_lr && g_pose_lr && g_betas_lr, "dir_mano_backward_pair: bad arguments");
    ManoBwdArgs a;
    for (int h = 0; h < hands; ++h) {
        const dir_mano_tables& t = tables_lr[h];
        if (int rc = mano::check_mano_tables(t, "dir_mano_backward_pair")) return rc;
        DIR_REQUIRE(!t.root_palm, "dir_mano_backward_pair: unsupported table flags (root_palm)");
        DIR_REQUIRE(pose_lr[h] && betas_lr[h] && g_pose_lr[h] && g_betas_lr[h] && pose_stride >= 51 && betas_stride >= 10 && g_pose_stride >= 51 && g_betas_stride >= 10,
                    "dir_mano_backward_pair: bad pointers / strides");
        const float* cam = cam_lr ? cam_lr[h] : nullptr;
        DIR_REQUIRE(!cam || (cam_stride >= 3 && (!g_cam_lr || !g_cam_lr[h] || g_cam_stride >= 3)), "dir_mano_backward_pair: bad cam strides");
        a.h[h] = ManoBwdHand{t, pose_lr[h], pose_stride, betas_lr[h], betas_stride, cam, cam_stride,
                             g_verts_lr ? g_verts_lr[h] : nullptr, g_joints_lr ? g_joints_lr[h] : nullptr,
                             g_joint_uv_lr ? g_joint_uv_lr[h] : nullptr, g_mesh_uv_lr ? g_mesh_uv_lr[h] : nullptr,
                             g_pose_lr[h], g_pose_stride, g_betas_lr[h], g_betas_stride, g_cam_lr ? g_cam_lr[h] : nullptr, g_cam_stride};
    }
    if (hands == 1) a.h[1] = a.h[0];
    DIR_LAUNCH(mano_backward_kernel, dim3(B, hands), dim3(BT), 0, (hipStream_t)stream, a);
    return check_launch("dir_mano_backward_pair");
}
