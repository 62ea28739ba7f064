// Temporal smoothing of tracked hands in MANO parameter space: dir_mano_para_smooth_step.  One launch is one frame of B sequences x `hands`:
// the root rotation is filtered on SO(3), the 15 finger joints per joint in axis-angle, the frame camera as three scalars, the betas are
// averaged over the first shape_frames usable frames and then frozen, and the mesh, the joints and the 2-D joints are regenerated from the
// filtered parameters by the MANO forward -- all inside the launch.  The rule, the order of every operation and the state layout are written
// out in include/dir_hip.h ("smoothing in MANO parameter space"); tests/helpers/para_smooth_ref.py restates it in torch.
//
//   mano_para_smooth_kernel   one 256-lane workgroup per (sequence, hand), the hand in LDS (29 KB) as in mano_fit.hip.  A few lanes do the
//                             scalar work (lane 64 the root, lanes 0..14 the fingers, 16..18 the camera, 32..41 the shape); the whole
//                             workgroup does the blend shapes, the skinning, the history shift and the reductions of the measures.
//
// The forward body restates mano.hip operation for operation, as mano_fit.hip does (a first usable frame gives dir_mano_forward's bits); the
// One-Euro arithmetic restates smooth.hip's.  No atomics, no workspace, no flags between workgroups, vector stores only: a (sequence, hand)
// gives the same bits in any slot of any batch and in either hand slot.
#include <math.h>

#include "dir_common.h"

namespace {

constexpr int NV = 778, NV3 = 2334, NV3P = 2336, NJ = 16, BT = 256;
constexpr int AGE_MAX = 1 << 30;                          // `age` and `run` saturate here
constexpr int O_J = NV3, O_PX = NV3 + 63;                 // a history row: verts [2334] | joints [63] | joints_px [42] (2439 floats, padded to 2440)
constexpr long long HIST = 2440 * 4;

// byte offsets inside one row of the state (dir_mano_para_smooth_state_bytes)
constexpr long long S_MEASURES = 0, S_Y1 = 64, S_Y2 = S_Y1 + HIST, S_X1 = S_Y2 + HIST, S_X2 = S_X1 + HIST, S_PREV = S_X2 + HIST, S_VEL = S_PREV + 256,
                    S_NSHAPE = S_VEL + 256, S_AGE = S_NSHAPE + 4, S_RUN = S_AGE + 4, S_COUNT = S_RUN + 4, S_ROW = S_COUNT + 4;
static_assert(S_ROW % 16 == 0 && S_ROW == 39632, "state row");

__constant__ int kReorderJs[21] = {0, 13, 14, 15, 16, 1, 2, 3, 17, 4, 5, 6, 18, 10, 11, 12, 19, 7, 8, 9, 20};
__constant__ int kTipss[2][5] = {{745, 317, 444, 556, 673}, {745, 317, 445, 556, 673}};

struct SmoothArgs {
    dir_mano_tables t[2];
    dir_mano_para_smooth_hand h[2];
    const int32_t* valid;
    double fps, d_cutoff;
    float min_cutoff, beta, rot_scale, cam_scale;
    int max_gap, shape_frames;
};

__device__ __forceinline__ bool finite(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

__device__ __forceinline__ float alpha(float r, float fc) {         // smooth.hip: r = 2 pi dt
#pragma clang fp contract(off)
    return 1.f / (1.f + 1.f / (r * fc));
}

__device__ __forceinline__ void normalize3s(float& x, float& y, float& z) {      // mano.hip: normalize3
#pragma clang fp contract(off)
    const float m = fmaxf(sqrtf(x * x + y * y + z * z), 1e-8f);
    x /= m; y /= m; z /= m;
}

// mano.hip's robust 6D -> rotation (row major, columns x', y', z) and its reflection flag
__device__ __forceinline__ void robust6d(const float* p, float* R, int& reflect) {
#pragma clang fp contract(off)
    float x0 = p[0], x1 = p[1], x2 = p[2], y0 = p[3], y1 = p[4], y2 = p[5];
    normalize3s(x0, x1, x2);
    normalize3s(y0, y1, y2);
    float m0 = x0 + y0, m1 = x1 + y1, m2 = x2 + y2;
    float o0 = x0 - y0, o1 = x1 - y1, o2 = x2 - y2;
    normalize3s(m0, m1, m2);
    normalize3s(o0, o1, o2);
    x0 = m0 + o0; x1 = m1 + o1; x2 = m2 + o2;
    y0 = m0 - o0; y1 = m1 - o1; y2 = m2 - o2;
    normalize3s(x0, x1, x2);
    normalize3s(y0, y1, y2);
    float z0 = x1 * y2 - x2 * y1, z1 = x2 * y0 - x0 * y2, z2 = x0 * y1 - x1 * y0;
    normalize3s(z0, z1, z2);
    R[0] = x0; R[1] = y0; R[2] = z0;
    R[3] = x1; R[4] = y1; R[5] = z1;
    R[6] = x2; R[7] = y2; R[8] = z2;
    const float det = x0 * (y1 * z2 - z1 * y2) - y0 * (x1 * z2 - z1 * x2) + z0 * (x1 * y2 - y1 * x2);
    reflect = det < 0.f ? 1 : 0;
}

// mano.hip's Rodrigues via quaternion.  OFFSET = true: the forward's own (angle = |v + 1e-8|); false: the root step's E, angle = |v| exactly and
// E = I at |v| == 0 -- the 1e-8 offset would bias every step by 1e-8 rad about a fixed direction (the step response is then not the scalar filter's)
template <bool OFFSET> __device__ __forceinline__ void rodrigues(float vx, float vy, float vz, float* R) {
#pragma clang fp contract(off)
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

// One-Euro on one point of D components (smooth.hip's walk_segment): x, the last output y1 and the speed estimate h, in LDS; y and h are updated
template <int D> __device__ __forceinline__ void one_euro_point(const float* x, const float* y1, float* h, float* y, float a_d, float r, float dt,
                                                                float min_cutoff, float beta, float scale) {
#pragma clang fp contract(off)
    float v2 = 0.f;
#pragma unroll
    for (int c = 0; c < D; ++c) {
        const float dx = (x[c] - y1[c]) / dt;
        const float dh = h[c] + a_d * (dx - h[c]);
        h[c] = dh;
        v2 += dh * dh;
    }
    const float fc = min_cutoff + beta * (scale * sqrtf(v2));
    const float al = alpha(r, fc);
#pragma unroll
    for (int c = 0; c < D; ++c) y[c] = y1[c] + al * (x[c] - y1[c]);
}

// one stream of n points x D components: the output is written, and on a usable row the second differences join the lane's partial sums (point
// order) and the history shifts.  yl: this frame's filtered values (LDS); xr: the raw stream's row or NULL (then its history and sum stay)
template <int D> __device__ __forceinline__ void walk_stream(int n, const float* yl, float* yo, const float* xr, float* y1, float* y2, float* x1, float* x2,
                                                             bool usable, bool jit, double& raw, double& fil) {
    for (int p = threadIdx.x; p < n; p += BT) {
        double r2 = 0., f2 = 0.;
#pragma unroll
        for (int c = 0; c < D; ++c) {
            const int i = p * D + c;
            const float yv = yl[i];
            yo[i] = yv;
            if (!usable) continue;
            const float y1v = y1[i], y2v = y2[i];
            const double df = (double)yv - 2. * (double)y1v + (double)y2v;
            f2 += df * df;
            y2[i] = y1v; y1[i] = yv;
            if (xr) {
                const float xv = xr[i], x1v = x1[i], x2v = x2[i];
                const double dr = (double)xv - 2. * (double)x1v + (double)x2v;
                r2 += dr * dr;
                x2[i] = x1v; x1[i] = xv;
            }
        }
        if (jit) { fil += sqrt(f2); if (xr) raw += sqrt(r2); }
    }
}

__device__ __forceinline__ double bone_length(const float* j, int p, int c) {
    const double d0 = (double)j[3 * c] - (double)j[3 * p], d1 = (double)j[3 * c + 1] - (double)j[3 * p + 1], d2 = (double)j[3 * c + 2] - (double)j[3 * p + 2];
    return sqrt(d0 * d0 + d1 * d1 + d2 * d2);
}

__global__ __launch_bounds__(BT) void mano_para_smooth_kernel(SmoothArgs args) {
    const dir_mano_tables& T = args.t[blockIdx.y];
    const dir_mano_para_smooth_hand& a = args.h[blockIdx.y];
    __shared__ float s_v[NV3P];          // v_shaped -> v_posed -> skinned -> centred vertices (in place)
    __shared__ float s_in[64];           // para[0:61] | cam_px
    __shared__ float s_prev[64];         // the state's last output: six | a_y1 | mean betas | c_y1
    __shared__ float s_vel[64];          // the state's speed estimates: w^ [3], 0 [3] | fingers [45] | unused [10] | camera [3]
    __shared__ float s_out[64];          // `smoothed`: six | a_y | b_y | c_y
    __shared__ float s_rot[135], s_pm[135], s_root[9], s_J[48];
    __shared__ float s_A[NJ * 12];
    __shared__ __attribute__((aligned(16))) float s_A2[NJ * 12];
    __shared__ float s_jtr[63], s_c[3], s_jo[63], s_px[42];
    __shared__ double s_red[8][BT];
    __shared__ int s_reflect, s_break;

    const int tid = threadIdx.x;
    const size_t b = blockIdx.x;
    const int center = T.center_idx;
    const float* s_full = s_out + 6;
    const float* s_beta = s_out + 51;
    unsigned char* st = static_cast<unsigned char*>(a.state) + b * (size_t)S_ROW;
    float* prev = reinterpret_cast<float*>(st + S_PREV);
    float* vel = reinterpret_cast<float*>(st + S_VEL);
    int* nshape_p = reinterpret_cast<int*>(st + S_NSHAPE);
    int* age_p = reinterpret_cast<int*>(st + S_AGE);
    int* run_p = reinterpret_cast<int*>(st + S_RUN);
    int* count_p = reinterpret_cast<int*>(st + S_COUNT);

    // ================================================================ step 0: the inputs; step 1: usable
    int bad = 0;
    if (tid < 64) {
        const float x = tid < 61 ? a.para[b * 64 + tid] : a.cam_px[b * 3 + (tid - 61)];
        s_in[tid] = x;
        bad = !finite(x);
        s_prev[tid] = prev[tid];
        s_vel[tid] = vel[tid];
    }
    if (tid == 0) s_break = 0;
    const int age = *age_p, run = *run_p, n_shape = *nshape_p;      // read by every lane; lane 0 writes them behind the last barrier
    bad = __syncthreads_or(bad);

    if (tid < 45) {                                                  // a_x = hands_mean + comps . pca (mano.hip)
        float acc = 0.f;
        for (int k = 0; k < 45; ++k) acc = fmaf(s_in[6 + k], T.comps[k * 45 + tid], acc);
        s_out[6 + tid] = T.hands_mean[tid] + acc;
    }
    if (tid == 64) {                                                 // R_x and its reflection flag
        int refl;
        robust6d(s_in, s_root, refl);
        s_reflect = refl;
    }
    if (tid >= 128 && tid < 134) s_out[tid - 128] = s_in[tid - 128];            // six, betas and camera pass through until a filter replaces them
    if (tid >= 128 + 51 && tid < 128 + 64) s_out[tid - 128] = s_in[tid - 128];
    __syncthreads();

    const bool usable = !(args.valid && !args.valid[b]) && !bad && !s_reflect;
    const bool init0 = age == 0 || age > args.max_gap;
    const double dt = (double)age / args.fps;
    const float dtf = (float)dt;
    const float r = (float)(6.283185307179586476925286766559 * dt);
    const float a_d = (float)(1. / (1. + 1. / (6.283185307179586476925286766559 * args.d_cutoff * dt)));

    // ================================================================ step 4, root rotation (one lane); a relative rotation about pi breaks
    if (tid == 64 && usable && !init0) {
#pragma clang fp contract(off)
        float Rp[9], D[9];
        int refl;
        robust6d(s_prev, Rp, refl);                                  // R_y1: the stored six through the same routine, the bits of the last frame
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) D[3 * i + j] = Rp[i] * s_root[j] + Rp[3 + i] * s_root[3 + j] + Rp[6 + i] * s_root[6 + j];
        const float s0 = 0.5f * (D[7] - D[5]), s1 = 0.5f * (D[2] - D[6]), s2 = 0.5f * (D[3] - D[1]);
        const float c = 0.5f * (((D[0] + D[4]) + D[8]) - 1.f);
        const float n = sqrtf(s0 * s0 + s1 * s1 + s2 * s2);
        if (n <= 1e-6f && c < 0.f) {
            s_break = 1;
        } else {
            float w[3] = {s0, s1, s2};
            if (!(n <= 1e-6f)) {
                const float k = atan2f(n, c) / n;
                w[0] = k * s0; w[1] = k * s1; w[2] = k * s2;
            }
            float v2 = 0.f;
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                const float dx = w[e] / dtf;
                const float dh = s_vel[e] + a_d * (dx - s_vel[e]);
                s_vel[e] = dh;
                v2 += dh * dh;
            }
            const float fc = args.min_cutoff + args.beta * (args.rot_scale * sqrtf(v2));
            const float al = alpha(r, fc);
            float E[9], Rt[9];
            rodrigues<false>(al * w[0], al * w[1], al * w[2], E);
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) Rt[3 * i + j] = Rp[3 * i] * E[j] + Rp[3 * i + 1] * E[3 + j] + Rp[3 * i + 2] * E[6 + j];
            s_out[0] = Rt[0]; s_out[1] = Rt[3]; s_out[2] = Rt[6];   // six = columns 0 and 1 of R_y1 . E
            s_out[3] = Rt[1]; s_out[4] = Rt[4]; s_out[5] = Rt[7];
            robust6d(s_out, s_root, refl);                           // R_y
        }
    }
    __syncthreads();
    const int mode = !usable ? 0 : (init0 || s_break) ? 2 : 1;       // `updated`

    // ================================================================ step 4, fingers and camera; step 5, shape
    if (mode == 1 && tid < 15)
        one_euro_point<3>(s_out + 6 + 3 * tid, s_prev + 6 + 3 * tid, s_vel + 6 + 3 * tid, s_out + 6 + 3 * tid, a_d, r, dtf, args.min_cutoff, args.beta, args.rot_scale);
    if (mode == 1 && tid >= 16 && tid < 19)
        one_euro_point<1>(s_out + 61 + (tid - 16), s_prev + 61 + (tid - 16), s_vel + 61 + (tid - 16), s_out + 61 + (tid - 16), a_d, r, dtf, args.min_cutoff, args.beta,
                          args.cam_scale);
    if (mode != 0 && args.shape_frames > 0 && tid >= 32 && tid < 42) {
#pragma clang fp contract(off)
        const int k = 51 + (tid - 32);
        float m = s_prev[k];
        if (n_shape < args.shape_frames) {
            const int n1 = n_shape + 1;
            const float bx = s_out[k];
            m = n1 == 1 ? bx : m + (bx - m) / (float)n1;
        }
        s_out[k] = m;
    }
    __syncthreads();
    if (tid < 64) {
        a.smoothed[b * 64 + tid] = s_out[tid];
        if (mode != 0) {
            if (tid < 51 || tid >= 61 || args.shape_frames > 0) prev[tid] = s_out[tid];
            vel[tid] = mode == 2 ? 0.f : s_vel[tid];
        }
    }

    // ================================================================ step 6: the forward from (R_y, a_y, b_y), as mano_forward_kernel from its shape blend on
    for (int i = tid; i < NV3; i += BT) {
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < 10; ++k) acc = fmaf(T.shapedirs_t[k * NV3P + i], s_beta[k], acc);
        s_v[i] = acc + T.v_template[i];
    }
    if (tid < 15) {
        float* R = s_rot + 9 * tid;
        rodrigues<true>(s_full[3 * tid], s_full[3 * tid + 1], s_full[3 * tid + 2], R);
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
        for (int q = 0; q < 3; ++q) {
            A[4 * q + 0] = s_root[3 * q + 0]; A[4 * q + 1] = s_root[3 * q + 1]; A[4 * q + 2] = s_root[3 * q + 2];
            A[4 * q + 3] = s_J[q];
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
            for (int q = 0; q < 3; ++q) {
                const float a0 = A[4 * q], a1 = A[4 * q + 1], a2 = A[4 * q + 2], a3 = A[4 * q + 3];
                N[4 * q + 0] = a0 * R[0] + a1 * R[3] + a2 * R[6];
                N[4 * q + 1] = a0 * R[1] + a1 * R[4] + a2 * R[7];
                N[4 * q + 2] = a0 * R[2] + a1 * R[5] + a2 * R[8];
                N[4 * q + 3] = a0 * t0 + a1 * t1 + a2 * t2 + a3;
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
        for (int q = 0; q < 3; ++q) {
            s_A2[12 * tid + 4 * q + 0] = A[4 * q + 0];
            s_A2[12 * tid + 4 * q + 1] = A[4 * q + 1];
            s_A2[12 * tid + 4 * q + 2] = A[4 * q + 2];
            s_A2[12 * tid + 4 * q + 3] = A[4 * q + 3] - (A[4 * q] * j0 + A[4 * q + 1] * j1 + A[4 * q + 2] * j2);
        }
    }
    __syncthreads();
    for (int v = tid; v < NV; v += BT) {
        const float4* wp = reinterpret_cast<const float4*>(T.weights + 16 * v);
        float w[16];
#pragma unroll
        for (int q = 0; q < 4; ++q) { const float4 t4 = wp[q]; w[4 * q] = t4.x; w[4 * q + 1] = t4.y; w[4 * q + 2] = t4.z; w[4 * q + 3] = t4.w; }
        float Tm[12];
#pragma unroll
        for (int e = 0; e < 12; ++e) Tm[e] = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const float4* ak = reinterpret_cast<const float4*>(s_A2 + 12 * k);
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const float4 t4 = ak[q];
                Tm[4 * q] = fmaf(t4.x, w[k], Tm[4 * q]); Tm[4 * q + 1] = fmaf(t4.y, w[k], Tm[4 * q + 1]);
                Tm[4 * q + 2] = fmaf(t4.z, w[k], Tm[4 * q + 2]); Tm[4 * q + 3] = fmaf(t4.w, w[k], Tm[4 * q + 3]);
            }
        }
        const float x = s_v[3 * v], y = s_v[3 * v + 1], z = s_v[3 * v + 2];
        s_v[3 * v + 0] = Tm[0] * x + Tm[1] * y + Tm[2] * z + Tm[3];
        s_v[3 * v + 1] = Tm[4] * x + Tm[5] * y + Tm[6] * z + Tm[7];
        s_v[3 * v + 2] = Tm[8] * x + Tm[9] * y + Tm[10] * z + Tm[11];
    }
    __syncthreads();
    if (tid < 21) {
        const int src = kReorderJs[tid];
        float x, y, z;
        if (src == 0 && T.root_palm) {
            x = (s_v[3 * 95] + s_v[3 * 22]) / 2; y = (s_v[3 * 95 + 1] + s_v[3 * 22 + 1]) / 2;
            z = (s_v[3 * 95 + 2] + s_v[3 * 22 + 2]) / 2;
        } else if (src < 16) { x = s_A[12 * src + 3]; y = s_A[12 * src + 7]; z = s_A[12 * src + 11]; }
        else { const int v = kTipss[T.side][src - 16]; x = s_v[3 * v]; y = s_v[3 * v + 1]; z = s_v[3 * v + 2]; }
        s_jtr[3 * tid] = x; s_jtr[3 * tid + 1] = y; s_jtr[3 * tid + 2] = z;
    }
    __syncthreads();
    if (tid < 3) s_c[tid] = center >= 0 ? s_jtr[3 * center + tid] : 0.f;
    __syncthreads();
    for (int i = tid; i < NV3; i += BT) s_v[i] = s_v[i] - s_c[i % 3];
    if (tid < 63) s_jo[tid] = s_jtr[tid] - s_c[tid % 3];
    if (tid >= 64 && tid < 64 + 42) {                                // joints_px = c_y[0] J.xy + c_y[1:3] (mano.hip's projection)
        const int i = tid - 64, j = i >> 1, c = i & 1;
        s_px[i] = s_out[61] * (s_jtr[3 * j + c] - s_c[c]) + (c ? s_out[63] : s_out[62]);
    }
    __syncthreads();

    // ================================================================ step 7: the measures; step 8: the history shift; the outputs
    const int run_new = mode == 0 ? 0 : mode == 2 ? 1 : (run < AGE_MAX ? run + 1 : AGE_MAX);
    const bool jit = run_new >= 3;
    float* y1 = reinterpret_cast<float*>(st + S_Y1);
    float* y2 = reinterpret_cast<float*>(st + S_Y2);
    float* x1 = reinterpret_cast<float*>(st + S_X1);
    float* x2 = reinterpret_cast<float*>(st + S_X2);
    const float* xv_r = a.raw_verts ? a.raw_verts + b * NV3 : nullptr;
    const float* xj_r = a.raw_joints ? a.raw_joints + b * 63 : nullptr;
    const float* xp_r = a.raw_joints_px ? a.raw_joints_px + b * 42 : nullptr;
    double sums[8] = {0., 0., 0., 0., 0., 0., 0., 0.};              // raw, filtered: mesh_xyz | joint_xyz | joints_px | bone flicker
    if (jit && tid < 20) {                                           // bone tid: finger f, link i; reads the joints' history before it shifts
        const int f = tid >> 2, i = tid & 3;
        const int p = i == 0 ? 0 : 4 * f + i, c = 4 * f + i + 1;
        sums[7] = fabs(bone_length(s_jo, p, c) - bone_length(y1 + O_J, p, c));
        if (xj_r) sums[6] = fabs(bone_length(xj_r, p, c) - bone_length(x1 + O_J, p, c));
    }
    __syncthreads();
    walk_stream<3>(NV, s_v, a.verts + b * NV3, xv_r, y1, y2, x1, x2, mode != 0, jit, sums[0], sums[1]);
    walk_stream<3>(21, s_jo, a.joints + b * 63, xj_r, y1 + O_J, y2 + O_J, x1 + O_J, x2 + O_J, mode != 0, jit, sums[2], sums[3]);
    walk_stream<2>(21, s_px, a.joints_px + b * 42, xp_r, y1 + O_PX, y2 + O_PX, x1 + O_PX, x2 + O_PX, mode != 0, jit, sums[4], sums[5]);
    if (jit) {                                                       // uniform over the workgroup
#pragma unroll
        for (int e = 0; e < 8; ++e) s_red[e][tid] = sums[e];
        __syncthreads();
        for (int o = BT / 2; o > 0; o >>= 1) {
            if (tid < o) {
#pragma unroll
                for (int e = 0; e < 8; ++e) s_red[e][tid] += s_red[e][tid + o];
            }
            __syncthreads();
        }
        if (tid < 8) reinterpret_cast<double*>(st + S_MEASURES)[tid] += s_red[tid][0];
    }
    if (tid == 0) {
        if (mode == 0) {
            if (age > 0) *age_p = age < AGE_MAX ? age + 1 : AGE_MAX;
            *run_p = 0;
        } else {
            *age_p = 1;
            *run_p = run_new;
            if (jit) *count_p += 1;
            if (args.shape_frames > 0 && n_shape < args.shape_frames) *nshape_p = n_shape + 1;
        }
        a.updated[b] = mode;
    }
}

}  // namespace

extern "C" long long dir_mano_para_smooth_state_bytes(long long* offsets) {
    if (offsets) {
        const long long v[DIR_MANO_PARA_SMOOTH_FIELDS] = {S_MEASURES, S_Y1, S_Y2, S_X1, S_X2, S_PREV, S_VEL, S_NSHAPE, S_AGE, S_RUN, S_COUNT};
        for (int i = 0; i < DIR_MANO_PARA_SMOOTH_FIELDS; ++i) offsets[i] = v[i];
    }
    return S_ROW;
}

extern "C" int dir_mano_para_smooth_step(const dir_mano_tables* tables_host, const dir_mano_para_smooth_hand* hands_host, const int32_t* valid,
                                         const dir_mano_para_smooth_opts* o, int hands, int B, void* stream) {
    DIR_REQUIRE(tables_host && hands_host && o, "dir_mano_para_smooth_step: null pointer");
    DIR_REQUIRE(hands == 1 || hands == 2, "dir_mano_para_smooth_step: bad args (hands %d outside 1..2)", hands);
    DIR_REQUIRE(B >= 1 && B <= DIR_CROP_MAX_BATCH, "dir_mano_para_smooth_step: bad args (B %d outside 1..%d)", B, DIR_CROP_MAX_BATCH);
    DIR_REQUIRE(isfinite(o->fps) && o->fps > 0. && isfinite(o->min_cutoff) && o->min_cutoff > 0. && isfinite(o->d_cutoff) && o->d_cutoff > 0. &&
                    isfinite(o->beta) && o->beta >= 0. && o->max_gap >= 1 && o->shape_frames >= 0,
                "dir_mano_para_smooth_step: bad args (non-positive rate: fps %g, min_cutoff %g, d_cutoff %g must be > 0, beta %g >= 0, max_gap %d >= 1, "
                "shape_frames %d >= 0)", o->fps, o->min_cutoff, o->d_cutoff, o->beta, o->max_gap, o->shape_frames);
    DIR_REQUIRE(isfinite(o->rot_speed_scale) && o->rot_speed_scale >= 0. && isfinite(o->cam_speed_scale) && o->cam_speed_scale >= 0.,
                "dir_mano_para_smooth_step: bad args (speed scales %g, %g must be finite and >= 0)", o->rot_speed_scale, o->cam_speed_scale);
    SmoothArgs a;
    for (int h = 0; h < 2; ++h) {
        const int s = h < hands ? h : 0;
        const dir_mano_tables& t = tables_host[s];
        const dir_mano_para_smooth_hand& x = hands_host[s];
        DIR_REQUIRE(x.para && x.cam_px && x.smoothed && x.verts && x.joints && x.joints_px && x.updated && x.state,
                    "dir_mano_para_smooth_step: null pointer (hand %d)", s);
        DIR_REQUIRE(t.shapedirs_t && t.posedirs_t && t.v_template && t.j_template && t.j_shapedirs && t.weights && t.hands_mean && t.comps,
                    "dir_mano_para_smooth_step: null table (hand %d)", s);
        DIR_REQUIRE(t.side == 0 || t.side == 1, "dir_mano_para_smooth_step: side must be 0 (right) or 1 (left)");
        DIR_REQUIRE(t.center_idx >= -1 && t.center_idx < 21, "dir_mano_para_smooth_step: center_idx out of range");
        DIR_REQUIRE(((uintptr_t)t.posedirs_t & 15) == 0 && ((uintptr_t)t.weights & 15) == 0,
                    "dir_mano_para_smooth_step: posedirs_t / weights must be 16-byte aligned");
        DIR_REQUIRE(((uintptr_t)x.state & 15) == 0, "dir_mano_para_smooth_step: the state must be 16-byte aligned");
        a.t[h] = t;
        a.h[h] = x;
    }
    a.valid = valid;
    a.fps = o->fps; a.d_cutoff = o->d_cutoff;
    a.min_cutoff = (float)o->min_cutoff; a.beta = (float)o->beta; a.rot_scale = (float)o->rot_speed_scale; a.cam_scale = (float)o->cam_speed_scale;
    a.max_gap = o->max_gap; a.shape_frames = o->shape_frames;
    DIR_LAUNCH(mano_para_smooth_kernel, dim3(B, hands), dim3(BT), 0, (hipStream_t)stream, a);
    return dir::check_launch("dir_mano_para_smooth_step");
}
