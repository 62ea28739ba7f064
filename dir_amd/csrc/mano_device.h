// The MANO layer on the device, in ONE place: manopth/manopth/manolayer.py:110-270 (+ rodrigues_layer.py:15-54, rot6d.py:26-60,
// tensutils.py:6-42) of the reference and its reverse.  Seven kernels call it: mano_forward_kernel (mano.hip), mano_backward_kernel
// (mano_bwd.hip), mano_fit_kernel (mano_fit.hip), mano_fit_seq_kernel (mano_fit_seq.hip), mano_fit_pair_kernel (mano_fit_pair.hip: two hands per 512-thread
// workgroup, the thread index taken modulo 256), mano_fit_start_kernel (mano_fit_start.hip) and mano_para_smooth_kernel (para_smooth.hip).  That mano_fit's iters = 0 and the
// smoother's first usable frame give dir_mano_forward's bits, and that the backward differentiates what the forward computes, holds
// because they run the same functions.
//
//   1. constants and per-thread primitives     every kernel
//   2. forward phases of a 256-thread workgroup holding one whole hand in LDS (struct Lds)        backward, fit, sequence fit, pair fit, fit start, smoother
//   3. backward phases of the same layout (struct BwdLds)                                         backward, fit, sequence fit, pair fit
//   4. the schedules: forward_schedule (the six kernels of 2) and DIR_MANO_BACKWARD_SCHEDULE (the four of 3)
//
// Everything is __forceinline__.  A phase holds no barrier; the two schedules hold the barriers of a whole pass and no arithmetic, so the
// synchronisation of the layer is read in layer 4 and every other __syncthreads() in the kernels.
// `#pragma clang fp contract(off)` is block-scoped, so a function carries the state of the block it replaced: the forward's robust 6D,
// Rodrigues and normalisation run uncontracted (they follow the reference's op sequence), the two chain rules at the end run contracted,
// their recomputation of the forward included -- that recomputation is therefore NOT robust6d() / rodrigues_quat() and is kept as it is.
// fp32 throughout; every sum in a fixed order.
#pragma once
#include "dir_common.h"

namespace dir {
namespace mano {

constexpr int NV = 778, NV3 = 2334, NV3P = 2336, NJ = 16;   // table rows padded to 2336 floats (16-B aligned)
constexpr int BT = 256;                                     // the workgroup of layers 2 and 3

static __constant__ int kReorderJ[21] = {0, 13, 14, 15, 16, 1, 2, 3, 17, 4, 5, 6, 18, 10, 11, 12, 19, 7, 8, 9, 20};
static __constant__ int kTips[2][5] = {{745, 317, 444, 556, 673}, {745, 317, 445, 556, 673}};

// ===================================================================================================== host: the tables' checks
// what every entry point requires of a dir_mano_tables; `who` = the entry point's name
inline int check_mano_tables(const dir_mano_tables& t, const char* who) {
    DIR_REQUIRE(t.shapedirs_t && t.posedirs_t && t.v_template && t.j_template && t.j_shapedirs && t.weights && t.hands_mean && t.comps,
                "%s: null table", who);
    DIR_REQUIRE(t.side == 0 || t.side == 1, "%s: side must be 0 (right) or 1 (left)", who);
    DIR_REQUIRE(t.center_idx >= -1 && t.center_idx < 21, "%s: center_idx out of range", who);
    DIR_REQUIRE(((uintptr_t)t.posedirs_t & 15) == 0 && ((uintptr_t)t.weights & 15) == 0, "%s: posedirs_t / weights must be 16-byte aligned", who);
    return DIR_OK;
}

// ===================================================================================================== 1. per-thread primitives
// rot6d.py:54-60: v / max(|v|, 1e-8).  No FMA contraction: the robust-6D construction is ill-conditioned for near-parallel inputs
// (x - y tiny), so follow the reference's op sequence exactly.  mag = the RAW magnitude |v|: the backward needs to know which branch of
// the clamp was taken (the forward ignores it)
__device__ __forceinline__ void normalize3(float& x, float& y, float& z, float& mag) {
#pragma clang fp contract(off)
    mag = sqrtf(x * x + y * y + z * z);
    const float m = fmaxf(mag, 1e-8f);
    x /= m; y /= m; z /= m;
}
// n = v / max(|v|, 1e-8): g v = (g - n (n . g)) / |v| where |v| >= 1e-8; in the clamped branch n = v / 1e-8 is linear in v and
// g v = g / 1e-8 without the projection (rot6d.py:54-60 under autograd: torch.max passes no gradient to |v| there).  A column shorter
// than 1e-8, or x^ - y^ of near-parallel columns, takes that branch.
__device__ __forceinline__ void normalize3_bwd(float nx, float ny, float nz, float mag, float& gx, float& gy, float& gz) {
    if (mag < 1e-8f) { gx /= 1e-8f; gy /= 1e-8f; gz /= 1e-8f; return; }
    const float d = nx * gx + ny * gy + nz * gz;
    gx = (gx - nx * d) / mag; gy = (gy - ny * d) / mag; gz = (gz - nz * d) / mag;
}

// robust 6D -> rotation (rot6d.py:26-51): R row major with columns (x', y', z); reflect = det R < 0 (the reference asserts det >= 0)
__device__ __forceinline__ void robust6d(const float* p, float* R, int& reflect) {
#pragma clang fp contract(off)
    float x0 = p[0], x1 = p[1], x2 = p[2], y0 = p[3], y1 = p[4], y2 = p[5], mg;
    normalize3(x0, x1, x2, mg);
    normalize3(y0, y1, y2, mg);
    float m0 = x0 + y0, m1 = x1 + y1, m2 = x2 + y2;
    float o0 = x0 - y0, o1 = x1 - y1, o2 = x2 - y2;
    normalize3(m0, m1, m2, mg);
    normalize3(o0, o1, o2, mg);
    x0 = m0 + o0; x1 = m1 + o1; x2 = m2 + o2;
    y0 = m0 - o0; y1 = m1 - o1; y2 = m2 - o2;
    normalize3(x0, x1, x2, mg);
    normalize3(y0, y1, y2, mg);
    float z0 = x1 * y2 - x2 * y1, z1 = x2 * y0 - x0 * y2, z2 = x0 * y1 - x1 * y0;
    normalize3(z0, z1, z2, mg);
    R[0] = x0; R[1] = y0; R[2] = z0;
    R[3] = x1; R[4] = y1; R[5] = z1;
    R[6] = x2; R[7] = y2; R[8] = z2;
    const float det = x0 * (y1 * z2 - z1 * y2) - y0 * (x1 * z2 - z1 * x2) + z0 * (x1 * y2 - y1 * x2);
    reflect = det < 0.f ? 1 : 0;
}

// Rodrigues via quaternion (rodrigues_layer.py:43-54, 15-40): axis-angle v[3] -> R[9] row major.  OFFSET = true: the layer's own
// (angle = |v + 1e-8|); false: angle = |v| exactly and R = I at |v| == 0, for the smoother's root step -- the 1e-8 offset would bias every
// step by 1e-8 rad about a fixed direction
template <bool OFFSET> __device__ __forceinline__ void rodrigues_quat(const float* v, float* R) {
#pragma clang fp contract(off)
    const float vx = v[0], vy = v[1], vz = v[2];
    float angle;
    if (OFFSET) {
        float ex = vx + 1e-8f, ey = vy + 1e-8f, ez = vz + 1e-8f;
        angle = sqrtf(ex * ex + ey * ey + ez * ez);
    } else {
        angle = sqrtf(vx * vx + vy * vy + vz * vz);
        if (angle == 0.f) {
#pragma unroll
            for (int e = 0; e < 9; ++e) R[e] = (e == 0 || e == 4 || e == 8) ? 1.f : 0.f;
            return;
        }
    }
    float ax = vx / angle, ay = vy / angle, az = vz / angle;
    float half = angle * 0.5f;
    float w = cosf(half), sn = sinf(half);
    float x = sn * ax, y = sn * ay, z = sn * az;
    float qn = sqrtf(w * w + x * x + y * y + z * z);
    w /= qn; x /= qn; y /= qn; z /= qn;
    float w2 = w * w, x2 = x * x, y2 = y * y, z2 = z * z;
    float wx = w * x, wy = w * y, wz = w * z, xy = x * y, xz = x * z, yz = y * z;
    R[0] = w2 + x2 - y2 - z2; R[1] = 2 * xy - 2 * wz;     R[2] = 2 * wy + 2 * xz;
    R[3] = 2 * wz + 2 * xy;   R[4] = w2 - x2 + y2 - z2;   R[5] = 2 * yz - 2 * wx;
    R[6] = 2 * xz - 2 * wy;   R[7] = 2 * wx + 2 * yz;     R[8] = w2 - x2 - y2 + z2;
}
// one articulated joint: its rotation and its row of the pose map R - I (tensutils.py:34-42)
__device__ __forceinline__ void joint_rotation(const float* v, float* R, float* pm) {
    rodrigues_quat<true>(v, R);
#pragma unroll
    for (int e = 0; e < 9; ++e) pm[e] = R[e] - ((e == 0 || e == 4 || e == 8) ? 1.f : 0.f);
}

// PCA coefficients -> component j of the 45 axis-angles (manolayer.py:131-144)
__device__ __forceinline__ float pca_axis_angle(const dir_mano_tables& t, const float* pca, int j) {
    float acc = 0.f;
    for (int k = 0; k < 45; ++k) acc = fmaf(pca[k], t.comps[k * 45 + j], acc);
    return t.hands_mean[j] + acc;
}

// coordinate o (= 3 joint + c) of the rest-pose joints (manolayer.py:183).  J = Jreg (v_template + shapedirs beta) is linear in beta:
// j_template = Jreg v_template [16,3] and j_shapedirs = Jreg shapedirs [16,3,10] are folded once at pack time (fp64), replacing 48 dot
// products of length 778 per sample by 48 of length 10
__device__ __forceinline__ float joint_regress(const dir_mano_tables& t, const float* beta, int o) {
    float acc = t.j_template[o];
#pragma unroll
    for (int k = 0; k < 10; ++k) acc = fmaf(t.j_shapedirs[o * 10 + k], beta[k], acc);
    return acc;
}

// kinematic chain (manolayer.py:192-229): finger fg owns joints 1 + 3 fg, 2 + 3 fg, 3 + 3 fg; finger 0 also writes the root's A_0 = [R_root | J_0].
// A: global transforms (top 3 rows), th_j joint order
__device__ __forceinline__ void chain_finger(int fg, const float* root, const float* J, const float* rot, float* As) {
    float A[12];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        A[4 * r + 0] = root[3 * r + 0]; A[4 * r + 1] = root[3 * r + 1]; A[4 * r + 2] = root[3 * r + 2];
        A[4 * r + 3] = J[r];
    }
    if (fg == 0) {
#pragma unroll
        for (int e = 0; e < 12; ++e) As[e] = A[e];
    }
    int parent = 0;
    for (int l = 0; l < 3; ++l) {
        const int j = 1 + 3 * fg + l;
        const float* R = rot + 9 * (j - 1);
        const float t0 = J[3 * j] - J[3 * parent], t1 = J[3 * j + 1] - J[3 * parent + 1], t2 = J[3 * j + 2] - J[3 * parent + 2];
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
        for (int e = 0; e < 12; ++e) { A[e] = N[e]; As[12 * j + e] = N[e]; }
        parent = j;
    }
}

// joint jt with the rest-pose joint removed: A' = A - pack(A.[J;0])  (manolayer.py:231-234)
__device__ __forceinline__ void a_prime(int jt, const float* As, const float* J, float* A2) {
    const float* A = As + 12 * jt;
    const float j0 = J[3 * jt], j1 = J[3 * jt + 1], j2 = J[3 * jt + 2];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        A2[12 * jt + 4 * r + 0] = A[4 * r + 0];
        A2[12 * jt + 4 * r + 1] = A[4 * r + 1];
        A2[12 * jt + 4 * r + 2] = A[4 * r + 2];
        A2[12 * jt + 4 * r + 3] = A[4 * r + 3] - (A[4 * r] * j0 + A[4 * r + 1] * j1 + A[4 * r + 2] * j2);
    }
}

__device__ __forceinline__ void load_weights(const float* weights, int v, float (&w)[16]) {
    const float4* wp = reinterpret_cast<const float4*>(weights + 16 * v);
#pragma unroll
    for (int q = 0; q < 4; ++q) { const float4 t4 = wp[q]; w[4 * q] = t4.x; w[4 * q + 1] = t4.y; w[4 * q + 2] = t4.z; w[4 * q + 3] = t4.w; }
}
// T = sum_k w[k] A'[k] (manolayer.py:236): A'[k] as three 16-byte LDS reads, A2 16-byte aligned
__device__ __forceinline__ void blend(const float (&w)[16], const float* A2, float (&T)[12]) {
#pragma unroll
    for (int e = 0; e < 12; ++e) T[e] = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const float4* ak = reinterpret_cast<const float4*>(A2 + 12 * k);
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const float4 t4 = ak[r];
            T[4 * r] = fmaf(t4.x, w[k], T[4 * r]); T[4 * r + 1] = fmaf(t4.y, w[k], T[4 * r + 1]);
            T[4 * r + 2] = fmaf(t4.z, w[k], T[4 * r + 2]); T[4 * r + 3] = fmaf(t4.w, w[k], T[4 * r + 3]);
        }
    }
}
__device__ __forceinline__ void blend(const float* weights, const float* A2, int v, float (&T)[12]) {
    float w[16];
    load_weights(weights, v, w);
    blend(w, A2, T);
}
// vert = T.[v_posed;1] (manolayer.py:245-246); src == dst skins in place
__device__ __forceinline__ void skin_vertex(const float (&T)[12], const float* src, float* dst, int v) {
    const float x = src[3 * v], y = src[3 * v + 1], z = src[3 * v + 2];
    dst[3 * v + 0] = T[0] * x + T[1] * y + T[2] * z + T[3];
    dst[3 * v + 1] = T[4] * x + T[5] * y + T[6] * z + T[7];
    dst[3 * v + 2] = T[8] * x + T[9] * y + T[10] * z + T[11];
}

// output joint jt before centring: one of the 16 chain joints or a fingertip vertex, reordered (manolayer.py:247-259); with root_palm the
// wrist is the midpoint of vertices 95 and 22.  vert: the skinned vertices; side, root_palm: the tables' (dir_mano_tables)
__device__ __forceinline__ void joint_source(int side, int root_palm, int jt, const float* As, const float* vert, float* jtr) {
    const int src = kReorderJ[jt];
    float x, y, z;
    if (src == 0 && root_palm) {
        x = (vert[3 * 95] + vert[3 * 22]) / 2; y = (vert[3 * 95 + 1] + vert[3 * 22 + 1]) / 2;
        z = (vert[3 * 95 + 2] + vert[3 * 22 + 2]) / 2;
    } else if (src < 16) { x = As[12 * src + 3]; y = As[12 * src + 7]; z = As[12 * src + 11]; }
    else { const int v = kTips[side][src - 16]; x = vert[3 * v]; y = vert[3 * v + 1]; z = vert[3 * v + 2]; }
    jtr[3 * jt] = x; jtr[3 * jt + 1] = y; jtr[3 * jt + 2] = z;
}

// ===================================================================================================== 2. forward phases, one hand per 256 threads
// What the phases share besides the vertices (the kernels keep those: the smoother one array in place, the other two v_posed and the skinned
// vertices) and the axis-angles (the smoother's live inside its `smoothed` row).
// The tables' side, center_idx and root_palm come as values.  The rule for a caller: read the three once at the kernel's top -- a scalar load
// inside a phase that a few threads run makes the whole workgroup wait for it at the next barrier (measured: 0.7 % of the backward and of the
// smoother).
// DIR_MANO_LDS(L, s) declares the arrays s_rot .. s_c as separate __shared__ objects and L as the phases' view of them.  Separate objects: as
// members of one __shared__ struct a store to A may alias rot or J for the compiler, and the serial chains (five threads, one LDS round trip
// after the other) then wait for every store before the next load (measured: 0.3 - 0.5 % of the smoother and the fit).  Their names matter:
// where the compiler places a kernel's LDS objects changes with their names, and the fit kernel measured 1.5 % slower with the same arrays
// named L_rot .. and G_gj .. than named s_rot .. beside its s_v, s_vert, s_gv (several builds each way; why the placement costs that is not
// known).  So a kernel passes the prefix its other arrays carry, and a change of these names is measured with tools/bench_mano_fit.py.
struct Lds {
    float* A2;              // [NJ * 12], 16-byte aligned: A' = A - pack(A.[J;0])
    float* rot;             // [15 * 9] rotation matrices (row major)
    float* pm;              // [135] pose map = R - I
    float* root;            // [9]
    float* J;               // [NJ * 3]
    float* A;               // [NJ * 12] global transforms (top 3 rows), th_j joint order
    float* jtr;             // [21 * 3]
    float* c;               // [3]
};
#define DIR_MANO_LDS(L, s)                                                                                  \
    __shared__ float s##_rot[135], s##_pm[135], s##_root[9], s##_J[48], s##_A[dir::mano::NJ * 12];          \
    __shared__ __attribute__((aligned(16))) float s##_A2[dir::mano::NJ * 12];                               \
    __shared__ float s##_jtr[63], s##_c[3];                                                                 \
    const dir::mano::Lds L = {s##_A2, s##_rot, s##_pm, s##_root, s##_J, s##_A, s##_jtr, s##_c}

// manolayer.py:180-182
__device__ __forceinline__ void shape_blend(const dir_mano_tables& t, const float* beta, float* v, int tid) {
    for (int i = tid; i < NV3; i += BT) {
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < 10; ++k) acc = fmaf(t.shapedirs_t[k * NV3P + i], beta[k], acc);
        v[i] = acc + t.v_template[i];
    }
}
__device__ __forceinline__ void joint_rotations(const Lds& L, const float* full, int tid) {
    if (tid < 15) joint_rotation(full + 3 * tid, L.rot + 9 * tid, L.pm + 9 * tid);
}
__device__ __forceinline__ void joint_regression(const Lds& L, const dir_mano_tables& t, const float* beta, int tid) {
    if (tid >= 128 && tid < 128 + NJ * 3) L.J[tid - 128] = joint_regress(t, beta, tid - 128);
}
// manolayer.py:186-187: one float4 column of the k-major table per thread and pass
__device__ __forceinline__ void pose_blend(const Lds& L, const dir_mano_tables& t, float* v, int tid) {
    for (int c4 = tid; c4 < NV3P / 4; c4 += BT) {
        const float4* pd = reinterpret_cast<const float4*>(t.posedirs_t) + c4;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 9
        for (int k = 0; k < 135; ++k) {
            const float4 p = pd[k * (NV3P / 4)];
            const float w = L.pm[k];
            acc.x = fmaf(p.x, w, acc.x); acc.y = fmaf(p.y, w, acc.y); acc.z = fmaf(p.z, w, acc.z); acc.w = fmaf(p.w, w, acc.w);
        }
        const int i = 4 * c4;
        v[i] += acc.x; v[i + 1] += acc.y;
        if (i + 2 < NV3) { v[i + 2] += acc.z; v[i + 3] += acc.w; }
    }
}
__device__ __forceinline__ void chain(const Lds& L, int tid) {
    if (tid < 5) chain_finger(tid, L.root, L.J, L.rot, L.A);
}
__device__ __forceinline__ void a_primes(const Lds& L, int tid) {
    if (tid < NJ) a_prime(tid, L.A, L.J, L.A2);
}
__device__ __forceinline__ void skinning(const Lds& L, const dir_mano_tables& t, const float* src, float* dst, int tid) {
    for (int v = tid; v < NV; v += BT) {
        float T[12];
        blend(t.weights, L.A2, v, T);
        skin_vertex(T, src, dst, v);
    }
}
__device__ __forceinline__ void joints(const Lds& L, int side, int root_palm, const float* vert, int tid) {
    if (tid < 21) joint_source(side, root_palm, tid, L.A, vert, L.jtr);
}
__device__ __forceinline__ void centre(const Lds& L, int center_idx, int tid) {       // manolayer.py:261-265
    if (tid < 3) L.c[tid] = center_idx >= 0 ? L.jtr[3 * center_idx + tid] : 0.f;
}

// ===================================================================================================== 3. backward phases, the same layout
// In: gj = g of the 21 output joints and gv = g of the skinned vertices, both already holding the projection's share, and sum3 = the sum of
// every position's g (the centre is subtracted from all of them).  Out: gvp = g v_posed, gJ, gfull, groot; the kernel stores what it wants.
struct BwdLds {             // as Lds: a view of separate __shared__ arrays, DIR_MANO_BWD_LDS(G, s)
    float* gj;              // [63]
    float* gAt;             // [48]
    float* gA2;             // [NJ * 12]
    float* gA;              // [NJ * 12]
    float* gJ;              // [48]
    float* gR;              // [135]
    float* gfull;           // [45]
    float (*part)[15];      // [5][15] per finger: g A_0 (12) | g J_0 (3) contributions
    float* groot;           // [9]
};
#define DIR_MANO_BWD_LDS(G, s)                                                                                                          \
    __shared__ float s##_gj[63], s##_gAt[48], s##_gA2[dir::mano::NJ * 12], s##_gA[dir::mano::NJ * 12], s##_gJ[48], s##_gR[135], s##_gfull[45]; \
    __shared__ float s##_part[5][15], s##_groot[9];                                                                                             \
    const dir::mano::BwdLds G = {s##_gj, s##_gAt, s##_gA2, s##_gA, s##_gJ, s##_gR, s##_gfull, s##_part, s##_groot}

__device__ __forceinline__ void centre_bwd(const BwdLds& G, int center_idx, const float* sum3, int tid) {
    if (tid < 3 && center_idx >= 0) G.gj[3 * center_idx + tid] -= sum3[tid];           // c = jtr[center] is subtracted from every output position
}
// joints back to their sources: chain joint translations, fingertip vertices, or the two palm vertices (half the gradient each).  gAt is zeroed before
__device__ __forceinline__ void joints_bwd(const BwdLds& G, int side, int root_palm, float* gv, int tid) {
    if (tid < 21) {
        const int src = kReorderJ[tid];
        if (src == 0 && root_palm) {
#pragma unroll
            for (int c = 0; c < 3; ++c) { const float h = G.gj[3 * tid + c] / 2; gv[3 * 95 + c] += h; gv[3 * 22 + c] += h; }
        } else if (src < 16) { G.gAt[3 * src] = G.gj[3 * tid]; G.gAt[3 * src + 1] = G.gj[3 * tid + 1]; G.gAt[3 * src + 2] = G.gj[3 * tid + 2]; }
        else {
            const int v = kTips[side][src - 16];
            gv[3 * v] += G.gj[3 * tid]; gv[3 * v + 1] += G.gj[3 * tid + 1]; gv[3 * v + 2] += G.gj[3 * tid + 2];
        }
    }
}
// skinning: vert = T.R v_posed + T.t  ->  g v_posed = T.R^T g vert
__device__ __forceinline__ void skinning_bwd(const Lds& L, const dir_mano_tables& t, const float* gv, float* gvp, int tid) {
    for (int v = tid; v < NV; v += BT) {
        float T[12];
        blend(t.weights, L.A2, v, T);
        const float gx = gv[3 * v], gy = gv[3 * v + 1], gz = gv[3 * v + 2];
        gvp[3 * v + 0] = T[0] * gx + T[4] * gy + T[8] * gz;
        gvp[3 * v + 1] = T[1] * gx + T[5] * gy + T[9] * gz;
        gvp[3 * v + 2] = T[2] * gx + T[6] * gy + T[10] * gz;
    }
    if (tid < 2) gvp[NV3 + tid] = 0.f;                 // padding of the 2336-float rows
}
// g A'[k][r][c] = sum_v w[v][k] g vert[v][r] (c < 3 ? v_posed[v][c] : 1): 192 reductions over the vertices
__device__ __forceinline__ void a_primes_grad(const BwdLds& G, const dir_mano_tables& t, const float* gv, const float* vp, int tid) {
    if (tid < NJ * 12) {
        const int k = tid / 12, e = tid - 12 * k, r = e >> 2, c = e & 3;
        float acc = 0.f;
        int v = 0;
        for (; v + 8 <= NV; v += 8) {                      // eight skinning weights in flight, accumulated in vertex order (the same sum as
            float w[8];                                    // 778 dependent global loads per thread)
#pragma unroll
            for (int u = 0; u < 8; ++u) w[u] = t.weights[16 * (v + u) + k];
#pragma unroll
            for (int u = 0; u < 8; ++u) acc = fmaf(w[u], gv[3 * (v + u) + r] * (c < 3 ? vp[3 * (v + u) + c] : 1.f), acc);
        }
        for (; v < NV; ++v) acc = fmaf(t.weights[16 * v + k], gv[3 * v + r] * (c < 3 ? vp[3 * v + c] : 1.f), acc);
        G.gA2[tid] = acc;
    }
}
// A' = [A.R | A.t - A.R J]  ->  g A.R = g A'.R - g A'.t (x) J ; g A.t = g A'.t (+ the joint's own gradient) ; g J = -A.R^T g A'.t
__device__ __forceinline__ void a_primes_bwd(const BwdLds& B, const Lds& L, int tid) {
    if (tid < NJ) {
        const float* A = L.A + 12 * tid;
        const float* G = B.gA2 + 12 * tid;
        const float j0 = L.J[3 * tid], j1 = L.J[3 * tid + 1], j2 = L.J[3 * tid + 2];
        const float t0 = G[3], t1 = G[7], t2 = G[11];
        const float tt[3] = {t0, t1, t2};
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            B.gA[12 * tid + 4 * r + 0] = G[4 * r + 0] - tt[r] * j0;
            B.gA[12 * tid + 4 * r + 1] = G[4 * r + 1] - tt[r] * j1;
            B.gA[12 * tid + 4 * r + 2] = G[4 * r + 2] - tt[r] * j2;
            B.gA[12 * tid + 4 * r + 3] = tt[r] + B.gAt[3 * tid + r];
        }
        B.gJ[3 * tid + 0] = -(A[0] * t0 + A[4] * t1 + A[8] * t2);
        B.gJ[3 * tid + 1] = -(A[1] * t0 + A[5] * t1 + A[9] * t2);
        B.gJ[3 * tid + 2] = -(A[2] * t0 + A[6] * t1 + A[10] * t2);
    }
}
// kinematic chain, leaf to root, one thread per finger: A_j = A_p [R_j | d_j], d_j = J_j - J_p
__device__ __forceinline__ void chain_bwd(const BwdLds& B, const Lds& L, int tid) {
    if (tid < 5) {
        float carry[12];                                 // gradient flowing into A_p from its child inside this finger
#pragma unroll
        for (int e = 0; e < 12; ++e) carry[e] = 0.f;
        for (int l = 2; l >= 0; --l) {
            const int j = 1 + 3 * tid + l, p = l == 0 ? 0 : j - 1;
            float G[12];
#pragma unroll
            for (int e = 0; e < 12; ++e) G[e] = B.gA[12 * j + e] + carry[e];
            const float* Ap = L.A + 12 * p;
            const float* R = L.rot + 9 * (j - 1);
            const float d0 = L.J[3 * j] - L.J[3 * p], d1 = L.J[3 * j + 1] - L.J[3 * p + 1], d2 = L.J[3 * j + 2] - L.J[3 * p + 2];
            // g R_j = A_p.R^T G.R
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    B.gR[9 * (j - 1) + 3 * r + c] = Ap[r] * G[c] + Ap[4 + r] * G[4 + c] + Ap[8 + r] * G[8 + c];
            // g d_j = A_p.R^T G.t
            const float gd0 = Ap[0] * G[3] + Ap[4] * G[7] + Ap[8] * G[11];
            const float gd1 = Ap[1] * G[3] + Ap[5] * G[7] + Ap[9] * G[11];
            const float gd2 = Ap[2] * G[3] + Ap[6] * G[7] + Ap[10] * G[11];
            B.gJ[3 * j] += gd0; B.gJ[3 * j + 1] += gd1; B.gJ[3 * j + 2] += gd2;
            // into the parent: g A_p.R = G.R R_j^T + G.t (x) d_j ; g A_p.t = G.t
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
                B.gJ[3 * p] -= gd0; B.gJ[3 * p + 1] -= gd1; B.gJ[3 * p + 2] -= gd2;     // p = j - 1: this finger's own joint
#pragma unroll
                for (int e = 0; e < 12; ++e) carry[e] = P[e];
            } else {
#pragma unroll
                for (int e = 0; e < 12; ++e) B.part[tid][e] = P[e];
                B.part[tid][12] = -gd0; B.part[tid][13] = -gd1; B.part[tid][14] = -gd2;
            }
        }
    }
}
// root: A_0 = [R_root | J_0]; fixed order over the five fingers
__device__ __forceinline__ void chain_root_bwd(const BwdLds& B, int tid) {
    if (tid < 15) {
        float acc = tid < 12 ? B.gA[tid] : 0.f;
        for (int f = 0; f < 5; ++f) acc += B.part[f][tid];
        if (tid < 12) B.gA[tid] = acc; else B.gJ[tid - 12] += acc;
    }
}
// g A_0 -> g J_0 (its translation) and g R_root
__device__ __forceinline__ void root_split_bwd(const BwdLds& B, int tid) {
    if (tid < 3) B.gJ[tid] += B.gA[4 * tid + 3];
    if (tid >= 64 && tid < 73) { const int e = tid - 64; B.groot[e] = B.gA[4 * (e / 3) + (e % 3)]; }
}

// <row, gvp> over one wave's lanes, before the reduction: eight table loads in flight, accumulated in order (the same sum)
__device__ __forceinline__ float row_dot(const float* row, const float* gvp, int lane) {
    float acc = 0.f;
    int i = lane;
    for (; i + 448 < NV3; i += 512) {
        float t[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) t[u] = row[i + 64 * u];
#pragma unroll
        for (int u = 0; u < 8; ++u) acc = fmaf(t[u], gvp[i + 64 * u], acc);
    }
    for (; i < NV3; i += 64) acc = fmaf(row[i], gvp[i], acc);
    return acc;
}
// pose blend shapes: g pm[k] = <posedirs_t[k], g v_posed>  (wave w: rows w, w + 4, ...), written over L.pm: the forward value is not needed
// any more, and g R_j = B.gR + this (pm = R - I).  WAVE_SUM: the caller's reducer, dir::wave_sum or dir::wave_sum_dpp (their last ulp differs)
template <float (*WAVE_SUM)(float)> __device__ __forceinline__ void pose_blend_bwd(const Lds& L, const dir_mano_tables& t, const float* gvp, int tid) {
    const int lane = tid & 63;
    for (int k = tid >> 6; k < 135; k += BT / 64) {
        const float acc = WAVE_SUM(row_dot(t.posedirs_t + (size_t)k * NV3P, gvp, lane));
        if (lane == 0) L.pm[k] = acc;
    }
}
// shape blend: g beta[k] = <shapedirs_t[k], g v_shaped> + <j_shapedirs[:, k], g J>   (g v_shaped = g v_posed); one wave, every lane gets the sum
template <float (*WAVE_SUM)(float)> __device__ __forceinline__ float shape_blend_bwd(const BwdLds& B, const dir_mano_tables& t, const float* gvp, int k, int lane) {
    float acc = row_dot(t.shapedirs_t + (size_t)k * NV3P, gvp, lane);
    if (lane < 48) acc = fmaf(t.j_shapedirs[lane * 10 + k], B.gJ[lane], acc);
    return WAVE_SUM(acc);
}
// PCA: full = mean + pca . comps  ->  g pca[k] = <comps[k], g full>
__device__ __forceinline__ float pca_bwd(const BwdLds& B, const dir_mano_tables& t, int k) {
    float acc = 0.f;
    for (int j = 0; j < 45; ++j) acc = fmaf(t.comps[k * 45 + j], B.gfull[j], acc);
    return acc;
}

// Rodrigues (via quaternion) chain rule of joint tid: g R_j (B.gR + the pose blend's share in L.pm) -> B.gfull.  Contracted, and so is its own
// recomputation of the quaternion: NOT rodrigues_quat()'s bits; leave it
__device__ __forceinline__ void rodrigues_bwd(const BwdLds& B, const Lds& L, const float* full, int tid) {
    if (tid < 15) {
        float g[9];
#pragma unroll
        for (int e = 0; e < 9; ++e) g[e] = B.gR[9 * tid + e] + L.pm[9 * tid + e];
        const float vx = full[3 * tid], vy = full[3 * tid + 1], vz = full[3 * tid + 2];
        const float ex = vx + 1e-8f, ey = vy + 1e-8f, ez = vz + 1e-8f;
        const float angle = sqrtf(ex * ex + ey * ey + ez * ez);
        const float ax = vx / angle, ay = vy / angle, az = vz / angle;
        const float half = angle * 0.5f;
        const float cw = cosf(half), sn = sinf(half);
        const float ux = sn * ax, uy = sn * ay, uz = sn * az;
        const float qn = sqrtf(cw * cw + ux * ux + uy * uy + uz * uz);
        const float w = cw / qn, x = ux / qn, y = uy / qn, z = uz / qn;
        // R(q) -> q
        float gw = 2 * w * (g[0] + g[4] + g[8]) + 2 * (-z * g[1] + y * g[2] + z * g[3] - x * g[5] - y * g[6] + x * g[7]);
        float gx = 2 * x * (g[0] - g[4] - g[8]) + 2 * (y * g[1] + z * g[2] + y * g[3] - w * g[5] + z * g[6] + w * g[7]);
        float gy = 2 * y * (-g[0] + g[4] - g[8]) + 2 * (x * g[1] + w * g[2] + x * g[3] + z * g[5] - w * g[6] + z * g[7]);
        float gz = 2 * z * (-g[0] - g[4] + g[8]) + 2 * (-w * g[1] + x * g[2] + w * g[3] + y * g[5] + x * g[6] + y * g[7]);
        // q = u / |u|
        const float dq = w * gw + x * gx + y * gy + z * gz;
        gw = (gw - w * dq) / qn; gx = (gx - x * dq) / qn; gy = (gy - y * dq) / qn; gz = (gz - z * dq) / qn;
        // u = (cos(half), sin(half) a)
        const float gsn = ax * gx + ay * gy + az * gz;
        const float gax = sn * gx, gay = sn * gy, gaz = sn * gz;
        const float ghalf = -sn * gw + cw * gsn;
        // a = v / angle, half = angle / 2, angle = |v + 1e-8|
        const float gangle = 0.5f * ghalf - (vx * gax + vy * gay + vz * gaz) / (angle * angle);
        B.gfull[3 * tid + 0] = gax / angle + gangle * ex / angle;
        B.gfull[3 * tid + 1] = gay / angle + gangle * ey / angle;
        B.gfull[3 * tid + 2] = gaz / angle + gangle * ez / angle;
    }
}
// robust 6D chain rule (one thread): groot[9] = g R_root -> g6[6].  Contracted: the sums, differences and the cross product of its own
// recomputation of the forward are NOT robust6d()'s bits; leave it
__device__ __forceinline__ void robust6d_bwd(const float* p, const float* groot, float* g6) {
    // forward again, keeping every normalisation's output and magnitude
    float xr0 = p[0], xr1 = p[1], xr2 = p[2], yr0 = p[3], yr1 = p[4], yr2 = p[5];
    float xh0 = xr0, xh1 = xr1, xh2 = xr2, yh0 = yr0, yh1 = yr1, yh2 = yr2, mxh, myh, mm, mo, mX, mY, mZ;
    normalize3(xh0, xh1, xh2, mxh);
    normalize3(yh0, yh1, yh2, myh);
    float m0 = xh0 + yh0, m1 = xh1 + yh1, m2 = xh2 + yh2, o0 = xh0 - yh0, o1 = xh1 - yh1, o2 = xh2 - yh2;
    normalize3(m0, m1, m2, mm);
    normalize3(o0, o1, o2, mo);
    float X0 = m0 + o0, X1 = m1 + o1, X2 = m2 + o2, Y0 = m0 - o0, Y1 = m1 - o1, Y2 = m2 - o2;
    normalize3(X0, X1, X2, mX);
    normalize3(Y0, Y1, Y2, mY);
    float Z0 = X1 * Y2 - X2 * Y1, Z1 = X2 * Y0 - X0 * Y2, Z2 = X0 * Y1 - X1 * Y0;
    normalize3(Z0, Z1, Z2, mZ);
    // g of the columns (row-major matrix with columns X, Y, Z)
    float gX0 = groot[0], gY0 = groot[1], gZ0 = groot[2], gX1 = groot[3], gY1 = groot[4], gZ1 = groot[5],
          gX2 = groot[6], gY2 = groot[7], gZ2 = groot[8];
    normalize3_bwd(Z0, Z1, Z2, mZ, gZ0, gZ1, gZ2);                      // Z = n(X x Y)
    // c = X x Y: g X += Y x g c ; g Y += g c x X
    gX0 += Y1 * gZ2 - Y2 * gZ1; gX1 += Y2 * gZ0 - Y0 * gZ2; gX2 += Y0 * gZ1 - Y1 * gZ0;
    gY0 += gZ1 * X2 - gZ2 * X1; gY1 += gZ2 * X0 - gZ0 * X2; gY2 += gZ0 * X1 - gZ1 * X0;
    normalize3_bwd(X0, X1, X2, mX, gX0, gX1, gX2);                      // X = n(m + o)
    normalize3_bwd(Y0, Y1, Y2, mY, gY0, gY1, gY2);                      // Y = n(m - o)
    float gm0 = gX0 + gY0, gm1 = gX1 + gY1, gm2 = gX2 + gY2, go0 = gX0 - gY0, go1 = gX1 - gY1, go2 = gX2 - gY2;
    normalize3_bwd(m0, m1, m2, mm, gm0, gm1, gm2);                      // m = n(x^ + y^)
    normalize3_bwd(o0, o1, o2, mo, go0, go1, go2);                      // o = n(x^ - y^)
    float gxh0 = gm0 + go0, gxh1 = gm1 + go1, gxh2 = gm2 + go2, gyh0 = gm0 - go0, gyh1 = gm1 - go1, gyh2 = gm2 - go2;
    normalize3_bwd(xh0, xh1, xh2, mxh, gxh0, gxh1, gxh2);
    normalize3_bwd(yh0, yh1, yh2, myh, gyh0, gyh1, gyh2);
    g6[0] = gxh0; g6[1] = gxh1; g6[2] = gxh2; g6[3] = gyh0; g6[4] = gyh1; g6[5] = gyh2;
}

// ===================================================================================================== 4. the schedules of a whole pass
// The phase calls in their order and the barriers between them, nothing else.  side, center_idx, root_palm: the values the kernel read at its
// top (layer 2's rule).  t is the thread index inside the hand's 256.

// joint_rotations .. centre.  Before it the kernel has written full (the 45 axis-angles), beta, L.root and v = the shape blend's output, with a
// barrier behind them where another thread wrote what joint_rotations or joint_regression reads; v becomes v_posed and vert the skinned vertices
// (vert == v skins in place: the smoother).  No barrier after centre: the kernel sets it, behind whatever else it writes for the next stage.
__device__ __forceinline__ void forward_schedule(const Lds& L, const dir_mano_tables& t, int side, int center_idx, int root_palm, const float* full,
                                                 const float* beta, float* v, float* vert, int tid) {
    joint_rotations(L, full, tid);
    joint_regression(L, t, beta, tid);
    __syncthreads();
    pose_blend(L, t, v, tid);
    chain(L, tid);
    __syncthreads();
    a_primes(L, tid);
    __syncthreads();
    skinning(L, t, v, vert, tid);
    __syncthreads();
    joints(L, side, root_palm, vert, tid);
    __syncthreads();
    centre(L, center_idx, tid);
}

// centre_bwd .. pose_blend_bwd and the barrier behind it.  In: layer 3's gj, gv, sum3 and a zeroed gAt, behind a barrier; vp = v_posed.  Out: gvp,
// G.gJ, G.gR, G.groot and the pose blend's share in L.pm, all visible to every thread.  WAVE_SUM: pose_blend_bwd's reducer, dir::wave_sum
// (mano_bwd.hip) or dir::wave_sum_dpp (the fits).
// A macro, not a function like forward_schedule: with these calls one inlining level further down the compiler forwards chain_bwd's stores to
// B.gJ differently and orders the operands of its sums differently, and dir_mano_backward_pair and every fit then give other bits than with the
// calls written out in the kernel (found on the MI355X; mano_backward_kernel's code differs in 2,800 lines of 5,600).  As a macro the
// kernels' code is what the written-out calls gave, instruction for instruction.  forward_schedule has no such effect.
#define DIR_MANO_BACKWARD_SCHEDULE(WAVE_SUM, G, L, t, side, center_idx, root_palm, sum3, vp, gv, gvp, tid) \
    do {                                                                                                   \
        dir::mano::centre_bwd(G, center_idx, sum3, tid);                                                   \
        __syncthreads();                                                                                   \
        dir::mano::joints_bwd(G, side, root_palm, gv, tid);                                                \
        __syncthreads();                                                                                   \
        dir::mano::skinning_bwd(L, t, gv, gvp, tid);                                                       \
        dir::mano::a_primes_grad(G, t, gv, vp, tid);                                                       \
        __syncthreads();                                                                                   \
        dir::mano::a_primes_bwd(G, L, tid);                                                                \
        __syncthreads();                                                                                   \
        dir::mano::chain_bwd(G, L, tid);                                                                   \
        __syncthreads();                                                                                   \
        dir::mano::chain_root_bwd(G, tid);                                                                 \
        __syncthreads();                                                                                   \
        dir::mano::root_split_bwd(G, tid);                                                                 \
        dir::mano::pose_blend_bwd<WAVE_SUM>(L, t, gvp, tid);                                               \
        __syncthreads();                                                                                   \
    } while (0)

}  // namespace mano

}  // namespace dir
