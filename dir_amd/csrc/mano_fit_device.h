// What the MANO fitting kernels share beyond the layer itself (mano_device.h): the residuals and their cotangents (steps 2 of the rule in
// include/dir_hip.h, "MANO fitting"), the mean squared residuals, and the priors' gradients with one Adam step of one component (steps 4 and 5).
// mano_fit_kernel (mano_fit.hip: the loop inside one launch) and mano_fit_seq_kernel (mano_fit_seq.hip: one launch per iteration, frames coupled
// in time) call them, which is why a sequence fitted with no temporal weight and a shape per frame gives dir_mano_fit's bits.
// mano_fit_pair_kernel (mano_fit_pair.hip: both hands of a pair in one workgroup) calls them too and adds the capsule term at the end of this file; with no
// capsule pair active it gives dir_mano_fit's bits for the same reason.
//
// As mano_device.h: everything is __forceinline__, a function holds NO barrier (the kernels keep every __syncthreads()), fp32 throughout, every sum
// in a fixed order.
#pragma once
#include "mano_device.h"

namespace dir {
namespace mano {
namespace fit {

// the per-thread part of step 2 for row b of hand `a`: the cotangents into gv (skinned vertices) and G.gj (joints, the projection's share included),
// and this thread's share of  red = sum g.x, g.y, g.z | g s | g tx, g ty | sq V | sq J, n J | sq U, n U
__device__ __forceinline__ void residuals(const dir_mano_fit_hand& a, size_t b, const Lds& L, const BwdLds& G, const float* vert, float* gv, const float* cam,
                                          bool use_v, bool use_j, bool use_uv, float kv, float kj, float kuv, int tid, float (&red)[11]) {
    const float sc = cam[0], tx = cam[1], ty = cam[2];
    for (int v = tid; v < NV; v += BT) {
        float gx = 0.f, gy = 0.f, gz = 0.f;
        if (use_v) {
            const float* t = a.verts_t + (b * NV + v) * 3;
            const float dx = (vert[3 * v] - L.c[0]) - t[0], dy = (vert[3 * v + 1] - L.c[1]) - t[1], dz = (vert[3 * v + 2] - L.c[2]) - t[2];
            gx = kv * dx; gy = kv * dy; gz = kv * dz;
            red[6] += dx * dx + dy * dy + dz * dz;
        }
        gv[3 * v] = gx; gv[3 * v + 1] = gy; gv[3 * v + 2] = gz;
        red[0] += gx; red[1] += gy; red[2] += gz;
    }
    if (tid < 21) {
        float gx = 0.f, gy = 0.f, gz = 0.f;
        const float jx = L.jtr[3 * tid] - L.c[0], jy = L.jtr[3 * tid + 1] - L.c[1], jz = L.jtr[3 * tid + 2] - L.c[2];
        if (use_j) {
            const float c = a.joints_conf ? a.joints_conf[b * 21 + tid] : 1.f;
            if (c > 0.f) {                                   // selected, never multiplied by 0: the target may hold NaN
                const float* t = a.joints_t + (b * 21 + tid) * 3;
                const float dx = jx - t[0], dy = jy - t[1], dz = jz - t[2], k = kj * c;
                gx = k * dx; gy = k * dy; gz = k * dz;
                red[7] += dx * dx + dy * dy + dz * dz; red[8] += 1.f;
            }
        }
        if (use_uv) {
            const float d = a.uv_conf ? a.uv_conf[b * 21 + tid] : 1.f;
            if (d > 0.f) {
                const float* t = a.uv_t + (b * 21 + tid) * 2;
                const float ex = (sc * jx + tx) - t[0], ey = (sc * jy + ty) - t[1], k = kuv * d;
                const float g0 = k * ex, g1 = k * ey;
                red[3] += g0 * jx + g1 * jy;
                red[4] += g0; red[5] += g1;
                gx = fmaf(sc, g0, gx); gy = fmaf(sc, g1, gy);
                red[9] += ex * ex + ey * ey; red[10] += 1.f;
            }
        }
        G.gj[3 * tid] = gx; G.gj[3 * tid + 1] = gy; G.gj[3 * tid + 2] = gz;
        red[0] += gx; red[1] += gy; red[2] += gz;
    }
}

// each wave's sum of red (DPP tree) into part[wave]: the six gradient sums always, the five of the mean squared residuals where wanted
__device__ __forceinline__ void residual_partials(const float (&red)[11], bool want_mse, float (*part)[11], int lane, int wave) {
#pragma unroll
    for (int e = 0; e < 6; ++e) { const float s = dir::wave_sum_dpp(red[e]); if (lane == 0) part[wave][e] = s; }
    if (want_mse) {
#pragma unroll
        for (int e = 6; e < 11; ++e) { const float s = dir::wave_sum_dpp(red[e]); if (lane == 0) part[wave][e] = s; }
    }
}

// term 0, 1, 2 = verts, joints, joint_uv: its mean squared residual from the block's sums (0 where absent or nothing is selected)
__device__ __forceinline__ float mean_sq(const float* sum, bool use_v, int term) {
    const float sq = term == 0 ? sum[6] : term == 1 ? sum[7] : sum[9];
    const float n = term == 0 ? (use_v ? 778.f : 0.f) : term == 1 ? sum[8] : sum[10];
    return n > 0.f ? sq / n : 0.f;
}

// step 4 for component i: the priors' gradients added to the backward's g, in the header's order
__device__ __forceinline__ float prior_gradient(int i, float g, float p, float anchor, float k_pca, float k_beta, float k_init) {
#pragma clang fp contract(off)
    if (i >= 6 && i < 51) g = g + k_pca * p;
    if (i >= 51 && i < 61) g = g + k_beta * p;
    g = g + k_init * (p - anchor);
    return g;
}

// step 5 for one component: pb1n / pb2n = the running products b1^t, b2^t AFTER this step.  Returns whether p, m and v are all finite.
__device__ __forceinline__ bool adam(float g, float lr, float b1, float b2, float eps, float pb1n, float pb2n, float& p, float& m, float& v) {
#pragma clang fp contract(off)
    m = b1 * m + (1.f - b1) * g;
    v = b2 * v + (1.f - b2) * (g * g);
    const float mhat = m / (1.f - pb1n), vhat = v / (1.f - pb2n);
    p = lr == 0.f ? p : p - (lr * mhat) / (sqrtf(vhat) + eps);
    return dir::finite(p) && dir::finite(m) && dir::finite(v);
}

__device__ __forceinline__ int group_of(int i) { return i < 6 ? 0 : i < 51 ? 1 : i < 61 ? 2 : 3; }

// ---- the capsule term of dir_mano_fit_pair (include/dir_hip.h, "MANO fitting: two hands together")
constexpr float kSegEps = 1e-12f;        // m^2: a segment shorter than 1 um is a point
constexpr float kMinDist = 1e-6f;        // m: below it two segments cross and the pair has no direction

__device__ __forceinline__ float clamp01(float x) { return x < 0.f ? 0.f : x > 1.f ? 1.f : x; }       // NaN stays NaN

// Ericson's closest points of the segments (A, B) and (C, D), the header's order of clamps and branches: the clamped parameters s, t, the
// distance d and n = (c1 - c2) / d.  No FMA contraction.
__device__ __forceinline__ void segment_closest(const float (&A)[3], const float (&B)[3], const float (&C)[3], const float (&D)[3], float& s, float& t,
                                                float (&n)[3], float& d) {
#pragma clang fp contract(off)
    const float d1[3] = {B[0] - A[0], B[1] - A[1], B[2] - A[2]}, d2[3] = {D[0] - C[0], D[1] - C[1], D[2] - C[2]};
    const float r[3] = {A[0] - C[0], A[1] - C[1], A[2] - C[2]};
    const float a = d1[0] * d1[0] + d1[1] * d1[1] + d1[2] * d1[2], e = d2[0] * d2[0] + d2[1] * d2[1] + d2[2] * d2[2];
    const float f = d2[0] * r[0] + d2[1] * r[1] + d2[2] * r[2];
    if (a <= kSegEps && e <= kSegEps) {
        s = 0.f; t = 0.f;
    } else if (a <= kSegEps) {
        s = 0.f; t = clamp01(f / e);
    } else {
        const float c = d1[0] * r[0] + d1[1] * r[1] + d1[2] * r[2];
        if (e <= kSegEps) {
            t = 0.f; s = clamp01(-c / a);
        } else {
            const float b = d1[0] * d2[0] + d1[1] * d2[1] + d1[2] * d2[2], den = a * e - b * b;
            s = den != 0.f ? clamp01((b * f - c * e) / den) : 0.f;
            t = (b * s + f) / e;
            if (t < 0.f) { t = 0.f; s = clamp01(-c / a); }
            else if (t > 1.f) { t = 1.f; s = clamp01((b - c) / a); }
        }
    }
    const float w[3] = {(A[0] + s * d1[0]) - (C[0] + t * d2[0]), (A[1] + s * d1[1]) - (C[1] + t * d2[1]), (A[2] + s * d1[2]) - (C[2] + t * d2[2])};
    d = sqrtf(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    n[0] = w[0] / d; n[1] = w[1] / d; n[2] = w[2] / d;
}

// one (left bone, right bone) pair: h (0 where the pair is skipped), whether it is active, whether it has no direction, and for an active pair the four
// endpoint gradients of step 2a
__device__ __forceinline__ void capsule_pair(const float (&A)[3], const float (&B)[3], const float (&C)[3], const float (&D)[3], float rsum, float k_col,
                                             float& h, bool& active, bool& nodir, float (&gA)[3], float (&gB)[3], float (&gC)[3], float (&gD)[3]) {
#pragma clang fp contract(off)
    float s, t, n[3], d;
    segment_closest(A, B, C, D, s, t, n, d);
    h = 0.f; active = false; nodir = false;
    if (!dir::finite(d)) { nodir = true; return; }
    const float hh = rsum - d;
    if (!(hh > 0.f)) return;
    h = hh;
    if (d < kMinDist) { nodir = true; return; }
    active = true;
    const float u = k_col * hh, ua = u * (1.f - s), ub = u * s, uc = u * (1.f - t), ud = u * t;
#pragma unroll
    for (int c = 0; c < 3; ++c) { gA[c] = -(ua * n[c]); gB[c] = -(ub * n[c]); gC[c] = uc * n[c]; gD[c] = ud * n[c]; }
}

}  // namespace fit
}  // namespace mano
}  // namespace dir
