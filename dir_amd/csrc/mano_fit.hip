// dir_mano_fit: MANO parameters fitted to meshes, 3-D joints and 2-D keypoints -- dir_mano_forward run the other way.  Per (sample, hand)
// the 64-vector p (pose 51 = 6D root | 45 PCA, betas 10, cam 3) is moved by `iters` Adam steps down the residual E(p) of
// include/dir_hip.h ("MANO fitting"); the rule, the order of every operation and the status bits are written out there.
//
// One 256-thread workgroup per (sample, hand), as mano_backward_kernel, and the iteration loop is INSIDE the kernel: the parameters, the
// Adam state, the posed and skinned vertices and their cotangents stay in LDS (46 KB) from the first iteration to the last; per
// iteration only the tables (L2 resident, shared by every workgroup) and the targets (9.3 KB per hand) are read from memory.  Composed from
// the existing launches one iteration is a forward, a few ATen residual operations, a backward and an optimiser step (measured: DESIGN.md, "MANO fitting").
//
// The forward and backward bodies restate mano.hip / mano_bwd.hip operation for operation (the outputs at iters = 0 are dir_mano_forward's
// bits); on top of mano_bwd.hip the root_palm wrist is differentiated (joint 0 = (v95 + v22) / 2 sends half its gradient to each vertex).
// fp32 throughout, every reduction in a fixed order, no atomics, no scratch buffer: a row gives the same bits in any slot of any batch and
// in either hand slot.
#include "dir_common.h"

namespace {

constexpr int NV = 778, NV3 = 2334, NV3P = 2336, NJ = 16, BT = 256, ST = DIR_MANO_FIT_STATE;

__constant__ int kReorderJf[21] = {0, 13, 14, 15, 16, 1, 2, 3, 17, 4, 5, 6, 18, 10, 11, 12, 19, 7, 8, 9, 20};
__constant__ int kTipsf[2][5] = {{745, 317, 444, 556, 673}, {745, 317, 445, 556, 673}};

struct FitArgs {
    dir_mano_tables t[2];
    dir_mano_fit_hand h[2];
    float kv, kj, kuv;                   // 2 w_v / 778, 2 w_j / 21, 2 w_uv / 21: formed in double on the host, rounded once
    float k_pca, k_beta, k_init;         // 2 w_pca, 2 w_beta, 2 w_init
    float lr[4], b1, b2, eps;
    int iters;
};

__device__ __forceinline__ bool finite(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

__device__ __forceinline__ void normalize3f(float& x, float& y, float& z, float& mag) {      // mano_bwd.hip: normalize3b
#pragma clang fp contract(off)
    mag = sqrtf(x * x + y * y + z * z);
    const float m = fmaxf(mag, 1e-8f);
    x /= m; y /= m; z /= m;
}
__device__ __forceinline__ void normalize3f_bwd(float nx, float ny, float nz, float mag, float& gx, float& gy, float& gz) {
    if (mag < 1e-8f) { gx /= 1e-8f; gy /= 1e-8f; gz /= 1e-8f; return; }
    const float d = nx * gx + ny * gy + nz * gz;
    gx = (gx - nx * d) / mag; gy = (gy - ny * d) / mag; gz = (gz - nz * d) / mag;
}

__global__ __launch_bounds__(BT) void mano_fit_kernel(FitArgs args) {
    const dir_mano_tables& T = args.t[blockIdx.y];
    const dir_mano_fit_hand& a = args.h[blockIdx.y];
    __shared__ float s_v[NV3P];          // v_posed
    __shared__ float s_vert[NV3P];       // skinned vertices (before centring)
    __shared__ float s_gv[NV3P];         // g of the skinned vertices
    __shared__ float s_gvp[NV3P];        // g of v_posed (= g of v_shaped)
    __shared__ float s_p[64], s_p0[64], s_anchor[64], s_m[64], s_vv[64], s_g[64];      // iterate, start, prior centre, Adam moments, gradient
    __shared__ float s_full[45], s_rot[135], s_pm[135], s_root[9], s_J[48];
    __shared__ float s_A[NJ * 12];
    __shared__ __attribute__((aligned(16))) float s_A2[NJ * 12];
    __shared__ float s_jtr[63], s_c[3];
    __shared__ float s_gj[63], s_gAt[48], s_gA2[NJ * 12], s_gA[NJ * 12], s_gJ[48], s_gR[135], s_gfull[45];
    __shared__ float s_part[5][15];
    __shared__ float s_red[4][11], s_sum[11], s_groot[9], s_mse[6];
    __shared__ int s_flag;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t b = blockIdx.x;
    const int center = T.center_idx;
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
        // ================================================================ forward at s_p (as mano_forward_kernel, one vertex part)
        if (tid < 45) {
            float acc = 0.f;
            for (int k = 0; k < 45; ++k) acc = fmaf(s_pose[6 + k], T.comps[k * 45 + tid], acc);
            s_full[tid] = T.hands_mean[tid] + acc;
        }
        for (int i = tid; i < NV3; i += BT) {
            float acc = 0.f;
#pragma unroll
            for (int k = 0; k < 10; ++k) acc = fmaf(T.shapedirs_t[k * NV3P + i], s_beta[k], acc);
            s_v[i] = acc + T.v_template[i];
        }
        if (tid == 64) {
#pragma clang fp contract(off)
            float x0 = s_pose[0], x1 = s_pose[1], x2 = s_pose[2], y0 = s_pose[3], y1 = s_pose[4], y2 = s_pose[5], mg;
            normalize3f(x0, x1, x2, mg);
            normalize3f(y0, y1, y2, mg);
            float m0 = x0 + y0, m1 = x1 + y1, m2 = x2 + y2;
            float o0 = x0 - y0, o1 = x1 - y1, o2 = x2 - y2;
            normalize3f(m0, m1, m2, mg);
            normalize3f(o0, o1, o2, mg);
            x0 = m0 + o0; x1 = m1 + o1; x2 = m2 + o2;
            y0 = m0 - o0; y1 = m1 - o1; y2 = m2 - o2;
            normalize3f(x0, x1, x2, mg);
            normalize3f(y0, y1, y2, mg);
            float z0 = x1 * y2 - x2 * y1, z1 = x2 * y0 - x0 * y2, z2 = x0 * y1 - x1 * y0;
            normalize3f(z0, z1, z2, mg);
            s_root[0] = x0; s_root[1] = y0; s_root[2] = z0;
            s_root[3] = x1; s_root[4] = y1; s_root[5] = z1;
            s_root[6] = x2; s_root[7] = y2; s_root[8] = z2;
            const float det = x0 * (y1 * z2 - z1 * y2) - y0 * (x1 * z2 - z1 * x2) + z0 * (x1 * y2 - y1 * x2);
            s_flag = det < 0.f ? 1 : 0;
        }
        __syncthreads();
        if (tid < 15) {
#pragma clang fp contract(off)
            float vx = s_full[3 * tid], vy = s_full[3 * tid + 1], vz = s_full[3 * tid + 2];
            float ex = vx + 1e-8f, ey = vy + 1e-8f, ez = vz + 1e-8f;
            float angle = sqrtf(ex * ex + ey * ey + ez * ez);
            float ax = vx / angle, ay = vy / angle, az = vz / angle;
            float half = angle * 0.5f;
            float w = cosf(half), sn = sinf(half);
            float x = sn * ax, y = sn * ay, z = sn * az;
            float qn = sqrtf(w * w + x * x + y * y + z * z);
            w /= qn; x /= qn; y /= qn; z /= qn;
            float w2 = w * w, x2 = x * x, y2 = y * y, z2 = z * z;
            float wx = w * x, wy = w * y, wz = w * z, xy = x * y, xz = x * z, yz = y * z;
            float* R = s_rot + 9 * tid;
            R[0] = w2 + x2 - y2 - z2; R[1] = 2 * xy - 2 * wz;     R[2] = 2 * wy + 2 * xz;
            R[3] = 2 * wz + 2 * xy;   R[4] = w2 - x2 + y2 - z2;   R[5] = 2 * yz - 2 * wx;
            R[6] = 2 * xz - 2 * wy;   R[7] = 2 * wx + 2 * yz;     R[8] = w2 - x2 - y2 + z2;
#pragma unroll
            for (int e = 0; e < 9; ++e) s_pm[9 * tid + e] = R[e] - ((e == 0 || e == 4 || e == 8) ? 1.f : 0.f);
        }
        if (tid >= 128 && tid < 128 + NJ * 3) {
            const int o = tid - 128;
            float acc = T.j_template[o];
#pragma unroll
            for (int k = 0; k < 10; ++k) acc = fmaf(T.j_shapedirs[o * 10 + k], s_beta[k], acc);
            s_J[o] = acc;
        }
        __syncthreads();
        for (int c4 = tid; c4 < NV3P / 4; c4 += BT) {
            const float4* pd = reinterpret_cast<const float4*>(T.posedirs_t) + c4;
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 9
            for (int k = 0; k < 135; ++k) {
                const float4 p = pd[k * (NV3P / 4)];
                const float w = s_pm[k];
                acc.x = fmaf(p.x, w, acc.x); acc.y = fmaf(p.y, w, acc.y); acc.z = fmaf(p.z, w, acc.z); acc.w = fmaf(p.w, w, acc.w);
            }
            const int i = 4 * c4;
            s_v[i] += acc.x; s_v[i + 1] += acc.y;
            if (i + 2 < NV3) { s_v[i + 2] += acc.z; s_v[i + 3] += acc.w; }
        }
        if (tid < 5) {
            float A[12];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                A[4 * r + 0] = s_root[3 * r + 0]; A[4 * r + 1] = s_root[3 * r + 1]; A[4 * r + 2] = s_root[3 * r + 2];
                A[4 * r + 3] = s_J[r];
            }
            if (tid == 0) {
#pragma unroll
                for (int e = 0; e < 12; ++e) s_A[e] = A[e];
            }
            int parent = 0;
            for (int l = 0; l < 3; ++l) {
                const int j = 1 + 3 * tid + l;
                const float* R = s_rot + 9 * (j - 1);
                const float t0 = s_J[3 * j] - s_J[3 * parent], t1 = s_J[3 * j + 1] - s_J[3 * parent + 1], t2 = s_J[3 * j + 2] - s_J[3 * parent + 2];
                float N[12];
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    const float a0 = A[4 * r], a1 = A[4 * r + 1], a2 = A[4 * r + 2], a3 = A[4 * r + 3];
                    N[4 * r + 0] = a0 * R[0] + a1 * R[3] + a2 * R[6];
                    N[4 * r + 1] = a0 * R[1] + a1 * R[4] + a2 * R[7];
                    N[4 * r + 2] = a0 * R[2] + a1 * R[5] + a2 * R[8];
                    N[4 * r + 3] = a0 * t0 + a1 * t1 + a2 * t2 + a3;
                }
#pragma unroll
                for (int e = 0; e < 12; ++e) { A[e] = N[e]; s_A[12 * j + e] = N[e]; }
                parent = j;
            }
        }
        __syncthreads();
        if (tid < NJ) {
            const float* A = s_A + 12 * tid;
            const float j0 = s_J[3 * tid], j1 = s_J[3 * tid + 1], j2 = s_J[3 * tid + 2];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                s_A2[12 * tid + 4 * r + 0] = A[4 * r + 0];
                s_A2[12 * tid + 4 * r + 1] = A[4 * r + 1];
                s_A2[12 * tid + 4 * r + 2] = A[4 * r + 2];
                s_A2[12 * tid + 4 * r + 3] = A[4 * r + 3] - (A[4 * r] * j0 + A[4 * r + 1] * j1 + A[4 * r + 2] * j2);
            }
        }
        __syncthreads();
        auto blend = [&](int v, float (&Tm)[12]) {            // T = sum_k w[v][k] A'[k]
            const float4* wp = reinterpret_cast<const float4*>(T.weights + 16 * v);
            float w[16];
#pragma unroll
            for (int q = 0; q < 4; ++q) { const float4 t4 = wp[q]; w[4 * q] = t4.x; w[4 * q + 1] = t4.y; w[4 * q + 2] = t4.z; w[4 * q + 3] = t4.w; }
#pragma unroll
            for (int e = 0; e < 12; ++e) Tm[e] = 0.f;
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const float4* ak = reinterpret_cast<const float4*>(s_A2 + 12 * k);
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    const float4 t4 = ak[r];
                    Tm[4 * r] = fmaf(t4.x, w[k], Tm[4 * r]); Tm[4 * r + 1] = fmaf(t4.y, w[k], Tm[4 * r + 1]);
                    Tm[4 * r + 2] = fmaf(t4.z, w[k], Tm[4 * r + 2]); Tm[4 * r + 3] = fmaf(t4.w, w[k], Tm[4 * r + 3]);
                }
            }
        };
        for (int v = tid; v < NV; v += BT) {
            float Tm[12];
            blend(v, Tm);
            const float x = s_v[3 * v], y = s_v[3 * v + 1], z = s_v[3 * v + 2];
            s_vert[3 * v + 0] = Tm[0] * x + Tm[1] * y + Tm[2] * z + Tm[3];
            s_vert[3 * v + 1] = Tm[4] * x + Tm[5] * y + Tm[6] * z + Tm[7];
            s_vert[3 * v + 2] = Tm[8] * x + Tm[9] * y + Tm[10] * z + Tm[11];
        }
        __syncthreads();
        if (tid < 21) {
            const int src = kReorderJf[tid];
            float x, y, z;
            if (src == 0 && T.root_palm) {
                x = (s_vert[3 * 95] + s_vert[3 * 22]) / 2; y = (s_vert[3 * 95 + 1] + s_vert[3 * 22 + 1]) / 2;
                z = (s_vert[3 * 95 + 2] + s_vert[3 * 22 + 2]) / 2;
            } else if (src < 16) { x = s_A[12 * src + 3]; y = s_A[12 * src + 7]; z = s_A[12 * src + 11]; }
            else { const int v = kTipsf[T.side][src - 16]; x = s_vert[3 * v]; y = s_vert[3 * v + 1]; z = s_vert[3 * v + 2]; }
            s_jtr[3 * tid] = x; s_jtr[3 * tid + 1] = y; s_jtr[3 * tid + 2] = z;
        }
        __syncthreads();
        if (tid < 3) s_c[tid] = center >= 0 ? s_jtr[3 * center + tid] : 0.f;
        __syncthreads();

        // ================================================================ residuals: the cotangents gV, gJ, gU; the mean squared residuals at p0 and at the end
        const bool last = it >= n_it, want_mse = it == 0 || last;
        const float sc = s_cam[0], tx = s_cam[1], ty = s_cam[2];
        float red[11] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};     // sum g.x, g.y, g.z | g s | g tx, g ty | sq V | sq J, n J | sq U, n U
        for (int v = tid; v < NV; v += BT) {
            float gx = 0.f, gy = 0.f, gz = 0.f;
            if (use_v) {
                const float* t = a.verts_t + (b * NV + v) * 3;
                const float dx = (s_vert[3 * v] - s_c[0]) - t[0], dy = (s_vert[3 * v + 1] - s_c[1]) - t[1], dz = (s_vert[3 * v + 2] - s_c[2]) - t[2];
                gx = args.kv * dx; gy = args.kv * dy; gz = args.kv * dz;
                red[6] += dx * dx + dy * dy + dz * dz;
            }
            s_gv[3 * v] = gx; s_gv[3 * v + 1] = gy; s_gv[3 * v + 2] = gz;
            red[0] += gx; red[1] += gy; red[2] += gz;
        }
        if (tid < 21) {
            float gx = 0.f, gy = 0.f, gz = 0.f;
            const float jx = s_jtr[3 * tid] - s_c[0], jy = s_jtr[3 * tid + 1] - s_c[1], jz = s_jtr[3 * tid + 2] - s_c[2];
            if (use_j) {
                const float c = a.joints_conf ? a.joints_conf[b * 21 + tid] : 1.f;
                if (c > 0.f) {                                   // selected, never multiplied by 0: the target may hold NaN
                    const float* t = a.joints_t + (b * 21 + tid) * 3;
                    const float dx = jx - t[0], dy = jy - t[1], dz = jz - t[2], k = args.kj * c;
                    gx = k * dx; gy = k * dy; gz = k * dz;
                    red[7] += dx * dx + dy * dy + dz * dz; red[8] += 1.f;
                }
            }
            if (use_uv) {
                const float d = a.uv_conf ? a.uv_conf[b * 21 + tid] : 1.f;
                if (d > 0.f) {
                    const float* t = a.uv_t + (b * 21 + tid) * 2;
                    const float ex = (sc * jx + tx) - t[0], ey = (sc * jy + ty) - t[1], k = args.kuv * d;
                    const float g0 = k * ex, g1 = k * ey;
                    red[3] += g0 * jx + g1 * jy;
                    red[4] += g0; red[5] += g1;
                    gx = fmaf(sc, g0, gx); gy = fmaf(sc, g1, gy);
                    red[9] += ex * ex + ey * ey; red[10] += 1.f;
                }
            }
            s_gj[3 * tid] = gx; s_gj[3 * tid + 1] = gy; s_gj[3 * tid + 2] = gz;
            red[0] += gx; red[1] += gy; red[2] += gz;
        }
#pragma unroll
        for (int e = 0; e < 6; ++e) { const float s = dir::wave_sum_dpp(red[e]); if (lane == 0) s_red[wave][e] = s; }
        if (want_mse) {
#pragma unroll
            for (int e = 6; e < 11; ++e) { const float s = dir::wave_sum_dpp(red[e]); if (lane == 0) s_red[wave][e] = s; }
        }
        if (tid < 48) { s_gAt[tid] = 0.f; }
        __syncthreads();
        if (tid < 11) s_sum[tid] = s_red[0][tid] + s_red[1][tid] + s_red[2][tid] + s_red[3][tid];
        __syncthreads();
        if (want_mse && tid < 3) {
            const float sq = tid == 0 ? s_sum[6] : tid == 1 ? s_sum[7] : s_sum[9];
            const float n = tid == 0 ? (use_v ? 778.f : 0.f) : tid == 1 ? s_sum[8] : s_sum[10];
            const float mse = n > 0.f ? sq / n : 0.f;
            if (it == 0) s_mse[tid] = mse;
            if (last) s_mse[3 + tid] = mse;
        }
        if (last) break;

        // ================================================================ backward (as mano_backward_kernel)
        if (tid < 3 && center >= 0) s_gj[3 * center + tid] -= s_sum[tid];           // c = jtr[center] is subtracted from every output position
        __syncthreads();
        if (tid < 21) {          // joints back to their sources: chain joint translations, fingertip vertices, or the two palm vertices
            const int src = kReorderJf[tid];
            if (src == 0 && T.root_palm) {
#pragma unroll
                for (int c = 0; c < 3; ++c) { const float h = s_gj[3 * tid + c] / 2; s_gv[3 * 95 + c] += h; s_gv[3 * 22 + c] += h; }
            } else if (src < 16) { s_gAt[3 * src] = s_gj[3 * tid]; s_gAt[3 * src + 1] = s_gj[3 * tid + 1]; s_gAt[3 * src + 2] = s_gj[3 * tid + 2]; }
            else {
                const int v = kTipsf[T.side][src - 16];
                s_gv[3 * v] += s_gj[3 * tid]; s_gv[3 * v + 1] += s_gj[3 * tid + 1]; s_gv[3 * v + 2] += s_gj[3 * tid + 2];
            }
        }
        __syncthreads();
        // ---- skinning: vert = T.R v_posed + T.t  ->  g v_posed = T.R^T g vert
        for (int v = tid; v < NV; v += BT) {
            float Tm[12];
            blend(v, Tm);
            const float gx = s_gv[3 * v], gy = s_gv[3 * v + 1], gz = s_gv[3 * v + 2];
            s_gvp[3 * v + 0] = Tm[0] * gx + Tm[4] * gy + Tm[8] * gz;
            s_gvp[3 * v + 1] = Tm[1] * gx + Tm[5] * gy + Tm[9] * gz;
            s_gvp[3 * v + 2] = Tm[2] * gx + Tm[6] * gy + Tm[10] * gz;
        }
        if (tid < 2) s_gvp[NV3 + tid] = 0.f;                 // padding of the 2336-float rows
        // ---- g A'[k][r][c] = sum_v w[v][k] g vert[v][r] (c < 3 ? v_posed[v][c] : 1): 192 reductions over the vertices
        if (tid < NJ * 12) {
            const int k = tid / 12, e = tid - 12 * k, r = e >> 2, c = e & 3;
            float acc = 0.f;
            int v = 0;
            for (; v + 8 <= NV; v += 8) {
                float w[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) w[u] = T.weights[16 * (v + u) + k];
#pragma unroll
                for (int u = 0; u < 8; ++u) acc = fmaf(w[u], s_gv[3 * (v + u) + r] * (c < 3 ? s_v[3 * (v + u) + c] : 1.f), acc);
            }
            for (; v < NV; ++v) acc = fmaf(T.weights[16 * v + k], s_gv[3 * v + r] * (c < 3 ? s_v[3 * v + c] : 1.f), acc);
            s_gA2[tid] = acc;
        }
        __syncthreads();
        // ---- A' = [A.R | A.t - A.R J]  ->  g A.R = g A'.R - g A'.t (x) J ; g A.t = g A'.t (+ the joint's own gradient) ; g J = -A.R^T g A'.t
        if (tid < NJ) {
            const float* A = s_A + 12 * tid;
            const float* G = s_gA2 + 12 * tid;
            const float j0 = s_J[3 * tid], j1 = s_J[3 * tid + 1], j2 = s_J[3 * tid + 2];
            const float t0 = G[3], t1 = G[7], t2 = G[11];
            const float tt[3] = {t0, t1, t2};
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                s_gA[12 * tid + 4 * r + 0] = G[4 * r + 0] - tt[r] * j0;
                s_gA[12 * tid + 4 * r + 1] = G[4 * r + 1] - tt[r] * j1;
                s_gA[12 * tid + 4 * r + 2] = G[4 * r + 2] - tt[r] * j2;
                s_gA[12 * tid + 4 * r + 3] = tt[r] + s_gAt[3 * tid + r];
            }
            s_gJ[3 * tid + 0] = -(A[0] * t0 + A[4] * t1 + A[8] * t2);
            s_gJ[3 * tid + 1] = -(A[1] * t0 + A[5] * t1 + A[9] * t2);
            s_gJ[3 * tid + 2] = -(A[2] * t0 + A[6] * t1 + A[10] * t2);
        }
        __syncthreads();
        // ---- kinematic chain, leaf to root: A_j = A_p [R_j | d_j], d_j = J_j - J_p
        if (tid < 5) {
            float carry[12];
#pragma unroll
            for (int e = 0; e < 12; ++e) carry[e] = 0.f;
            for (int l = 2; l >= 0; --l) {
                const int j = 1 + 3 * tid + l, p = l == 0 ? 0 : j - 1;
                float G[12];
#pragma unroll
                for (int e = 0; e < 12; ++e) G[e] = s_gA[12 * j + e] + carry[e];
                const float* Ap = s_A + 12 * p;
                const float* R = s_rot + 9 * (j - 1);
                const float d0 = s_J[3 * j] - s_J[3 * p], d1 = s_J[3 * j + 1] - s_J[3 * p + 1], d2 = s_J[3 * j + 2] - s_J[3 * p + 2];
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int c = 0; c < 3; ++c)
                        s_gR[9 * (j - 1) + 3 * r + c] = Ap[r] * G[c] + Ap[4 + r] * G[4 + c] + Ap[8 + r] * G[8 + c];
                const float gd0 = Ap[0] * G[3] + Ap[4] * G[7] + Ap[8] * G[11];
                const float gd1 = Ap[1] * G[3] + Ap[5] * G[7] + Ap[9] * G[11];
                const float gd2 = Ap[2] * G[3] + Ap[6] * G[7] + Ap[10] * G[11];
                s_gJ[3 * j] += gd0; s_gJ[3 * j + 1] += gd1; s_gJ[3 * j + 2] += gd2;
                float P[12];
                const float dd[3] = {d0, d1, d2};
#pragma unroll
                for (int r = 0; r < 3; ++r) {
#pragma unroll
                    for (int c = 0; c < 3; ++c)
                        P[4 * r + c] = G[4 * r] * R[3 * c] + G[4 * r + 1] * R[3 * c + 1] + G[4 * r + 2] * R[3 * c + 2] + G[4 * r + 3] * dd[c];
                    P[4 * r + 3] = G[4 * r + 3];
                }
                if (l > 0) {
                    s_gJ[3 * p] -= gd0; s_gJ[3 * p + 1] -= gd1; s_gJ[3 * p + 2] -= gd2;
#pragma unroll
                    for (int e = 0; e < 12; ++e) carry[e] = P[e];
                } else {
#pragma unroll
                    for (int e = 0; e < 12; ++e) s_part[tid][e] = P[e];
                    s_part[tid][12] = -gd0; s_part[tid][13] = -gd1; s_part[tid][14] = -gd2;
                }
            }
        }
        __syncthreads();
        if (tid < 15) {          // root: A_0 = [R_root | J_0]; fixed order over the five fingers
            float acc = tid < 12 ? s_gA[tid] : 0.f;
            for (int f = 0; f < 5; ++f) acc += s_part[f][tid];
            if (tid < 12) s_gA[tid] = acc; else s_gJ[tid - 12] += acc;
        }
        __syncthreads();
        if (tid < 3) s_gJ[tid] += s_gA[4 * tid + 3];
        if (tid >= 64 && tid < 73) { const int e = tid - 64; s_groot[e] = s_gA[4 * (e / 3) + (e % 3)]; }
        // ---- pose blend shapes: g pm[k] = <posedirs_t[k], g v_posed>  (wave w: rows w, w + 4, ...), added to g R (pm = R - I)
        for (int k = wave; k < 135; k += BT / 64) {
            const float* row = T.posedirs_t + (size_t)k * NV3P;
            float acc = 0.f;
            int i = lane;
            for (; i + 448 < NV3; i += 512) {                  // eight table loads in flight, accumulated in order
                float t[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) t[u] = row[i + 64 * u];
#pragma unroll
                for (int u = 0; u < 8; ++u) acc = fmaf(t[u], s_gvp[i + 64 * u], acc);
            }
            for (; i < NV3; i += 64) acc = fmaf(row[i], s_gvp[i], acc);
            acc = dir::wave_sum_dpp(acc);
            if (lane == 0) s_pm[k] = acc;                     // (s_pm re-used: the next forward writes it again)
        }
        __syncthreads();
        // ---- Rodrigues (via quaternion) chain rule per joint; robust 6D chain rule for the root
        if (tid < 15) {
            float g[9];
#pragma unroll
            for (int e = 0; e < 9; ++e) g[e] = s_gR[9 * tid + e] + s_pm[9 * tid + e];
            const float vx = s_full[3 * tid], vy = s_full[3 * tid + 1], vz = s_full[3 * tid + 2];
            const float ex = vx + 1e-8f, ey = vy + 1e-8f, ez = vz + 1e-8f;
            const float angle = sqrtf(ex * ex + ey * ey + ez * ez);
            const float ax = vx / angle, ay = vy / angle, az = vz / angle;
            const float half = angle * 0.5f;
            const float cw = cosf(half), sn = sinf(half);
            const float ux = sn * ax, uy = sn * ay, uz = sn * az;
            const float qn = sqrtf(cw * cw + ux * ux + uy * uy + uz * uz);
            const float w = cw / qn, x = ux / qn, y = uy / qn, z = uz / qn;
            float gw = 2 * w * (g[0] + g[4] + g[8]) + 2 * (-z * g[1] + y * g[2] + z * g[3] - x * g[5] - y * g[6] + x * g[7]);
            float gx = 2 * x * (g[0] - g[4] - g[8]) + 2 * (y * g[1] + z * g[2] + y * g[3] - w * g[5] + z * g[6] + w * g[7]);
            float gy = 2 * y * (-g[0] + g[4] - g[8]) + 2 * (x * g[1] + w * g[2] + x * g[3] + z * g[5] - w * g[6] + z * g[7]);
            float gz = 2 * z * (-g[0] - g[4] + g[8]) + 2 * (-w * g[1] + x * g[2] + w * g[3] + y * g[5] + x * g[6] + y * g[7]);
            const float dq = w * gw + x * gx + y * gy + z * gz;
            gw = (gw - w * dq) / qn; gx = (gx - x * dq) / qn; gy = (gy - y * dq) / qn; gz = (gz - z * dq) / qn;
            const float gsn = ax * gx + ay * gy + az * gz;
            const float gax = sn * gx, gay = sn * gy, gaz = sn * gz;
            const float ghalf = -sn * gw + cw * gsn;
            const float gangle = 0.5f * ghalf - (vx * gax + vy * gay + vz * gaz) / (angle * angle);
            s_gfull[3 * tid + 0] = gax / angle + gangle * ex / angle;
            s_gfull[3 * tid + 1] = gay / angle + gangle * ey / angle;
            s_gfull[3 * tid + 2] = gaz / angle + gangle * ez / angle;
        }
        if (tid == 64) {
            float xr0 = s_pose[0], xr1 = s_pose[1], xr2 = s_pose[2], yr0 = s_pose[3], yr1 = s_pose[4], yr2 = s_pose[5];
            float xh0 = xr0, xh1 = xr1, xh2 = xr2, yh0 = yr0, yh1 = yr1, yh2 = yr2, mxh, myh, mm, mo, mX, mY, mZ;
            normalize3f(xh0, xh1, xh2, mxh);
            normalize3f(yh0, yh1, yh2, myh);
            float m0 = xh0 + yh0, m1 = xh1 + yh1, m2 = xh2 + yh2, o0 = xh0 - yh0, o1 = xh1 - yh1, o2 = xh2 - yh2;
            normalize3f(m0, m1, m2, mm);
            normalize3f(o0, o1, o2, mo);
            float X0 = m0 + o0, X1 = m1 + o1, X2 = m2 + o2, Y0 = m0 - o0, Y1 = m1 - o1, Y2 = m2 - o2;
            normalize3f(X0, X1, X2, mX);
            normalize3f(Y0, Y1, Y2, mY);
            float Z0 = X1 * Y2 - X2 * Y1, Z1 = X2 * Y0 - X0 * Y2, Z2 = X0 * Y1 - X1 * Y0;
            normalize3f(Z0, Z1, Z2, mZ);
            float gX0 = s_groot[0], gY0 = s_groot[1], gZ0 = s_groot[2], gX1 = s_groot[3], gY1 = s_groot[4], gZ1 = s_groot[5],
                  gX2 = s_groot[6], gY2 = s_groot[7], gZ2 = s_groot[8];
            normalize3f_bwd(Z0, Z1, Z2, mZ, gZ0, gZ1, gZ2);
            gX0 += Y1 * gZ2 - Y2 * gZ1; gX1 += Y2 * gZ0 - Y0 * gZ2; gX2 += Y0 * gZ1 - Y1 * gZ0;
            gY0 += gZ1 * X2 - gZ2 * X1; gY1 += gZ2 * X0 - gZ0 * X2; gY2 += gZ0 * X1 - gZ1 * X0;
            normalize3f_bwd(X0, X1, X2, mX, gX0, gX1, gX2);
            normalize3f_bwd(Y0, Y1, Y2, mY, gY0, gY1, gY2);
            float gm0 = gX0 + gY0, gm1 = gX1 + gY1, gm2 = gX2 + gY2, go0 = gX0 - gY0, go1 = gX1 - gY1, go2 = gX2 - gY2;
            normalize3f_bwd(m0, m1, m2, mm, gm0, gm1, gm2);
            normalize3f_bwd(o0, o1, o2, mo, go0, go1, go2);
            float gxh0 = gm0 + go0, gxh1 = gm1 + go1, gxh2 = gm2 + go2, gyh0 = gm0 - go0, gyh1 = gm1 - go1, gyh2 = gm2 - go2;
            normalize3f_bwd(xh0, xh1, xh2, mxh, gxh0, gxh1, gxh2);
            normalize3f_bwd(yh0, yh1, yh2, myh, gyh0, gyh1, gyh2);
            s_g[0] = gxh0; s_g[1] = gxh1; s_g[2] = gxh2; s_g[3] = gyh0; s_g[4] = gyh1; s_g[5] = gyh2;
        }
        // ---- shape blend: g beta[k] = <shapedirs_t[k], g v_shaped> + <j_shapedirs[:, k], g J>   (g v_shaped = g v_posed)
        for (int k = wave; k < 10; k += BT / 64) {
            const float* row = T.shapedirs_t + (size_t)k * NV3P;
            float acc = 0.f;
            int i = lane;
            for (; i + 448 < NV3; i += 512) {
                float t[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) t[u] = row[i + 64 * u];
#pragma unroll
                for (int u = 0; u < 8; ++u) acc = fmaf(t[u], s_gvp[i + 64 * u], acc);
            }
            for (; i < NV3; i += 64) acc = fmaf(row[i], s_gvp[i], acc);
            if (lane < 48) acc = fmaf(T.j_shapedirs[lane * 10 + k], s_gJ[lane], acc);
            acc = dir::wave_sum_dpp(acc);
            if (lane == 0) s_g[51 + k] = acc;
        }
        if (tid >= 128 && tid < 131) s_g[61 + tid - 128] = s_sum[3 + tid - 128];
        __syncthreads();
        // ---- PCA: full = mean + pca . comps  ->  g pca[k] = <comps[k], g full>
        if (tid < 45) {
            float acc = 0.f;
            for (int t = 0; t < 45; ++t) acc = fmaf(T.comps[tid * 45 + t], s_gfull[t], acc);
            s_g[6 + tid] = acc;
        }
        __syncthreads();

        // ================================================================ the priors' gradients and one Adam step (include/dir_hip.h gives this order)
        float p_new = 0.f, m_new = 0.f, v_new = 0.f;
        int bad = 0;
        const float pb1n = pb1 * args.b1, pb2n = pb2 * args.b2;
        if (tid < 64) {
#pragma clang fp contract(off)
            const float p = s_p[tid];
            float g = s_g[tid];
            if (tid >= 6 && tid < 51) g = g + args.k_pca * p;
            if (tid >= 51 && tid < 61) g = g + args.k_beta * p;
            g = g + args.k_init * (p - s_anchor[tid]);
            m_new = args.b1 * s_m[tid] + (1.f - args.b1) * g;
            v_new = args.b2 * s_vv[tid] + (1.f - args.b2) * (g * g);
            const float lr = args.lr[tid < 6 ? 0 : tid < 51 ? 1 : tid < 61 ? 2 : 3];
            const float mhat = m_new / (1.f - pb1n), vhat = v_new / (1.f - pb2n);
            p_new = lr == 0.f ? p : p - (lr * mhat) / (sqrtf(vhat) + args.eps);
            bad = !finite(p_new) || !finite(m_new) || !finite(v_new);
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
        for (int i = tid; i < NV3; i += BT) a.verts[b * NV3 + i] = p0_bad ? 0.f : s_vert[i] - s_c[i % 3];
    if (a.joints && tid < 63) a.joints[b * 63 + tid] = p0_bad ? 0.f : s_jtr[tid] - s_c[tid % 3];
    if (a.joint_uv && tid >= 64 && tid < 64 + 42) {
        const int i = tid - 64, j = i >> 1, c = i & 1;
        a.joint_uv[b * 42 + i] = p0_bad ? 0.f : s_cam[0] * (s_jtr[3 * j + c] - s_c[c]) + (c ? s_cam[2] : s_cam[1]);
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
        DIR_REQUIRE(t.shapedirs_t && t.posedirs_t && t.v_template && t.j_template && t.j_shapedirs && t.weights && t.hands_mean && t.comps,
                    "dir_mano_fit: null table");
        DIR_REQUIRE((t.side == 0 || t.side == 1) && t.center_idx >= -1 && t.center_idx < 21, "dir_mano_fit: bad table flags");
        DIR_REQUIRE(((uintptr_t)t.posedirs_t & 15) == 0 && ((uintptr_t)t.weights & 15) == 0, "dir_mano_fit: posedirs_t / weights must be 16-byte aligned");
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
