// What the MANO fitting kernels share beyond the layer itself (mano_device.h): the residuals and their cotangents (steps 2 of the rule in
// include/dir_hip.h, "MANO fitting"), the mean squared residuals, and the priors' gradients with one Adam step of one component (steps 4 and 5).
// mano_fit_kernel (mano_fit.hip: the loop inside one launch) and mano_fit_seq_kernel (mano_fit_seq.hip: one launch per iteration, frames coupled
// in time) call them, which is why a sequence fitted with no temporal weight and a shape per frame gives dir_mano_fit's bits.
// mano_fit_pair_kernel (mano_fit_pair.hip: both hands of a pair in one workgroup) calls them too and adds the capsule term at the end of this file; with no
// capsule pair active it gives dir_mano_fit's bits for the same reason.
//
// Around those, what the fit kernels would otherwise each write out: the scaled rule and the argument checks of the three entry points (host), the
// scan of the targets for non-finite values (also mano_fit_start_kernel's), the row and the Adam clock to and from LDS, the tail of the gradient behind
// mano_device.h's backward schedule, and the outputs at the final iterate.
//
// As mano_device.h: everything is __forceinline__, no function here holds a barrier (the kernels keep every __syncthreads() outside the two schedules),
// fp32 throughout, every sum in a fixed order, and a function carries the contraction state of the block it replaced.
#pragma once
#include <initializer_list>

#include "mano_device.h"

namespace dir {
namespace mano {
namespace fit {

// ===================================================================================================== host: the rule, scaled, and the checks
// what the kernels read of a dir_mano_fit_opts; FitArgs, SeqArgs and PairArgs embed it
struct Rule {
    float kv, kj, kuv;                   // 2 w_v / 778, 2 w_j / 21, 2 w_uv / 21: formed in double on the host, rounded once
    float k_pca, k_beta, k_init;         // 2 w_pca, 2 w_beta, 2 w_init
    float lr[4], b1, b2, eps;
    int iters;
};

// checks o and fills r.  `more`: the entry point's further weights and rates, held to the same range; `who` = the entry point's name
inline int check_opts(const dir_mano_fit_opts& o, std::initializer_list<float> more, const char* who, Rule& r) {
    DIR_REQUIRE(o.iters >= 0, "%s: iters must be >= 0", who);
    bool in_range = true;
    for (float w : {o.w_verts, o.w_joints, o.w_uv, o.w_pca, o.w_beta, o.w_init, o.lr[0], o.lr[1], o.lr[2], o.lr[3]}) in_range &= w >= 0.f && w <= 3.4e38f;
    for (float w : more) in_range &= w >= 0.f && w <= 3.4e38f;
    DIR_REQUIRE(in_range, "%s: weights and learning rates must be finite and >= 0", who);
    DIR_REQUIRE(o.b1 >= 0.f && o.b1 < 1.f && o.b2 >= 0.f && o.b2 < 1.f && o.eps > 0.f, "%s: need 0 <= b1, b2 < 1 and eps > 0", who);
    r.kv = (float)(2.0 * o.w_verts / 778.0); r.kj = (float)(2.0 * o.w_joints / 21.0); r.kuv = (float)(2.0 * o.w_uv / 21.0);
    r.k_pca = 2.f * o.w_pca; r.k_beta = 2.f * o.w_beta; r.k_init = 2.f * o.w_init;
    for (int g = 0; g < 4; ++g) r.lr[g] = o.lr[g];
    r.b1 = o.b1; r.b2 = o.b2; r.eps = o.eps; r.iters = o.iters;
    return DIR_OK;
}

inline int check_hand(const dir_mano_fit_hand& f, const char* who) {
    DIR_REQUIRE(f.p0 && f.p_out, "%s: null pointer (p0 / p_out)", who);
    DIR_REQUIRE((!f.joints_conf || f.joints_t) && (!f.uv_conf || f.uv_t), "%s: confidences without their target", who);
    return DIR_OK;
}

// ===================================================================================================== device
// whether this thread met a non-finite value among the targets in use of row b (a confidence of 0 selects its entry out, which may then hold NaN).
// Hand: dir_mano_fit_hand or dir_mano_fit_start_hand
template <class Hand> __device__ __forceinline__ int targets_nonfinite(const Hand& a, size_t b, int tid) {
    int bad_t = 0;
    if (a.verts_t)
        for (int i = tid; i < NV3; i += BT) bad_t |= !dir::finite(a.verts_t[b * NV3 + i]);
    if (tid < 21) {
        if (a.joints_t) {
            const float c = a.joints_conf ? a.joints_conf[b * 21 + tid] : 1.f;
            if (c > 0.f) {
                const float* t = a.joints_t + (b * 21 + tid) * 3;
                bad_t |= !dir::finite(c) || !dir::finite(t[0]) || !dir::finite(t[1]) || !dir::finite(t[2]);
            }
        }
        if (a.uv_t) {
            const float d = a.uv_conf ? a.uv_conf[b * 21 + tid] : 1.f;
            if (d > 0.f) {
                const float* t = a.uv_t + (b * 21 + tid) * 2;
                bad_t |= !dir::finite(d) || !dir::finite(t[0]) || !dir::finite(t[1]);
            }
        }
    }
    return bad_t;
}

// the Adam clock of row b of a state [B][DIR_MANO_FIT_STATE]: b1^t, b2^t as running fp32 products and t (every thread carries the same values);
// state may be NULL, and a row with t = 0 reads as 1, 1, 0 whatever it holds
__device__ __forceinline__ void load_clock(const float* state, size_t b, float& pb1, float& pb2, int& t_step) {
    pb1 = 1.f; pb2 = 1.f; t_step = 0;
    if (state) {
        t_step = __float_as_int(state[b * DIR_MANO_FIT_STATE + 130]);
        if (t_step > 0) { pb1 = state[b * DIR_MANO_FIT_STATE + 128]; pb2 = state[b * DIR_MANO_FIT_STATE + 129]; }
    }
}
__device__ __forceinline__ void store_clock(float* state, size_t b, float pb1, float pb2, int t_step) {      // one thread
    state[b * DIR_MANO_FIT_STATE + 128] = pb1; state[b * DIR_MANO_FIT_STATE + 129] = pb2;
    state[b * DIR_MANO_FIT_STATE + 130] = __int_as_float(t_step); state[b * DIR_MANO_FIT_STATE + 131] = 0.f;
}

// row b into LDS: the start (also the first iterate), the prior centre and the Adam moments.  Returns whether this thread's p0 or anchor is non-finite
__device__ __forceinline__ int load_row(const dir_mano_fit_hand& a, size_t b, float* p0, float* p, float* anchor, float* m, float* vv, int tid) {
    int bad_p = 0;
    if (tid < 64) {
        const float x = a.p0[b * 64 + tid];
        const float an = a.anchor ? a.anchor[b * 64 + tid] : x;
        p0[tid] = x; p[tid] = x; anchor[tid] = an;
        m[tid] = a.state ? a.state[b * DIR_MANO_FIT_STATE + tid] : 0.f;
        vv[tid] = a.state ? a.state[b * DIR_MANO_FIT_STATE + 64 + tid] : 0.f;
        bad_p = !dir::finite(x) || !dir::finite(an);
    }
    return bad_p;
}
// and back: p_out and the moments; a row that passed through returns p0 and leaves its state alone
__device__ __forceinline__ void store_row(const dir_mano_fit_hand& a, size_t b, bool pass, const float* p0, const float* p, const float* m, const float* vv,
                                          int tid) {
    if (tid < 64) {
        a.p_out[b * 64 + tid] = pass ? p0[tid] : p[tid];
        if (a.state && !pass) { a.state[b * DIR_MANO_FIT_STATE + tid] = m[tid]; a.state[b * DIR_MANO_FIT_STATE + 64 + tid] = vv[tid]; }
    }
}

// behind rodrigues_bwd and the root's robust6d_bwd, which stay in the kernels (the sequence fit adds its temporal term to G.groot between the two, and
// this order of the three is the one the kernels' code was generated for): the shape's ten sums into g[51..60], one wave per sum, and the camera's
// gradient g[61..63] = sum[3..5]
__device__ __forceinline__ void gradient_tail(const BwdLds& G, const dir_mano_tables& t, const float* gvp, const float* sum, float* g, int tid) {
    const int lane = tid & 63;
    for (int k = tid >> 6; k < 10; k += BT / 64) {
        const float acc = shape_blend_bwd<dir::wave_sum_dpp>(G, t, gvp, k, lane);
        if (lane == 0) g[51 + k] = acc;
    }
    if (tid >= 128 && tid < 131) g[61 + tid - 128] = sum[3 + tid - 128];
}

// verts, joints and joint_uv of row b at the iterate the last forward ran at (each optional); zeros where p0 was non-finite.  Contracted, as mano.hip's projection
__device__ __forceinline__ void write_outputs(const dir_mano_fit_hand& a, size_t b, const Lds& L, const float* vert, const float* cam, bool p0_bad, int tid) {
    if (a.verts)
        for (int i = tid; i < NV3; i += BT) a.verts[b * NV3 + i] = p0_bad ? 0.f : vert[i] - L.c[i % 3];
    if (a.joints && tid < 63) a.joints[b * 63 + tid] = p0_bad ? 0.f : L.jtr[tid] - L.c[tid % 3];
    if (a.joint_uv && tid >= 64 && tid < 64 + 42) {
        const int i = tid - 64, j = i >> 1, c = i & 1;
        a.joint_uv[b * 42 + i] = p0_bad ? 0.f : cam[0] * (L.jtr[3 * j + c] - L.c[c]) + (c ? cam[2] : cam[1]);
    }
}

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
