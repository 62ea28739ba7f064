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
// The forward is mano_device.h's forward schedule over the phases mano.hip runs (a first usable frame gives dir_mano_forward's bits), skinning in place; the
// One-Euro arithmetic restates smooth.hip's.  No atomics, no workspace, no flags between workgroups, vector stores only: a (sequence, hand)
// gives the same bits in any slot of any batch and in either hand slot.
#include <math.h>

#include "mano_device.h"

namespace {

using namespace dir::mano;
using dir::finite;

constexpr int AGE_MAX = 1 << 30;                          // `age` and `run` saturate here
constexpr int O_J = NV3, O_PX = NV3 + 63;                 // a history row: verts [2334] | joints [63] | joints_px [42] (2439 floats, padded to 2440)
constexpr long long HIST = 2440 * 4;

// byte offsets inside one row of the state (dir_mano_para_smooth_state_bytes)
constexpr long long S_MEASURES = 0, S_Y1 = 64, S_Y2 = S_Y1 + HIST, S_X1 = S_Y2 + HIST, S_X2 = S_X1 + HIST, S_PREV = S_X2 + HIST, S_VEL = S_PREV + 256,
                    S_NSHAPE = S_VEL + 256, S_AGE = S_NSHAPE + 4, S_RUN = S_AGE + 4, S_COUNT = S_RUN + 4, S_ROW = S_COUNT + 4;
static_assert(S_ROW % 16 == 0 && S_ROW == 39632, "state row");

struct SmoothArgs {
    dir_mano_tables t[2];
    dir_mano_para_smooth_hand h[2];
    const int32_t* valid;
    double fps, d_cutoff;
    float min_cutoff, beta, rot_scale, cam_scale;
    int max_gap, shape_frames;
};

__device__ __forceinline__ float alpha(float r, float fc) {         // smooth.hip: r = 2 pi dt
#pragma clang fp contract(off)
    return 1.f / (1.f + 1.f / (r * fc));
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
    const int side = T.side, center = T.center_idx, root_palm = T.root_palm;       // read once, here (mano_device.h, layer 2)
    __shared__ float s_v[NV3P];          // v_shaped -> v_posed -> skinned -> centred vertices (in place)
    __shared__ float s_in[64];           // para[0:61] | cam_px
    __shared__ float s_prev[64];         // the state's last output: six | a_y1 | mean betas | c_y1
    __shared__ float s_vel[64];          // the state's speed estimates: w^ [3], 0 [3] | fingers [45] | unused [10] | camera [3]
    __shared__ float s_out[64];          // `smoothed`: six | a_y | b_y | c_y
    DIR_MANO_LDS(L, s);
    __shared__ float s_jo[63], s_px[42];
    __shared__ double s_red[8][BT];
    __shared__ int s_reflect, s_break;

    const int tid = threadIdx.x;
    const size_t b = blockIdx.x;
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

    if (tid < 45) s_out[6 + tid] = pca_axis_angle(T, s_in + 6, tid);       // a_x = hands_mean + comps . pca
    if (tid == 64) {                                                 // R_x and its reflection flag
        int refl;
        robust6d(s_in, L.root, refl);
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
            for (int j = 0; j < 3; ++j) D[3 * i + j] = Rp[i] * L.root[j] + Rp[3 + i] * L.root[3 + j] + Rp[6 + i] * L.root[6 + j];
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
            const float step[3] = {al * w[0], al * w[1], al * w[2]};
            rodrigues_quat<false>(step, E);                          // angle = |v| exactly, E = I at 0: see rodrigues_quat
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) Rt[3 * i + j] = Rp[3 * i] * E[j] + Rp[3 * i + 1] * E[3 + j] + Rp[3 * i + 2] * E[6 + j];
            s_out[0] = Rt[0]; s_out[1] = Rt[3]; s_out[2] = Rt[6];   // six = columns 0 and 1 of R_y1 . E
            s_out[3] = Rt[1]; s_out[4] = Rt[4]; s_out[5] = Rt[7];
            robust6d(s_out, L.root, refl);                           // R_y
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

    // ================================================================ step 6: the forward from (R_y, a_y, b_y): mano_device.h's shape blend and forward schedule
    shape_blend(T, s_beta, s_v, tid);
    forward_schedule(L, T, side, center, root_palm, s_full, s_beta, s_v, s_v, tid);      // skinning in place
    __syncthreads();
    for (int i = tid; i < NV3; i += BT) s_v[i] = s_v[i] - L.c[i % 3];
    if (tid < 63) s_jo[tid] = L.jtr[tid] - L.c[tid % 3];
    if (tid >= 64 && tid < 64 + 42) {                                // joints_px = c_y[0] J.xy + c_y[1:3] (mano.hip's projection)
        const int i = tid - 64, j = i >> 1, c = i & 1;
        s_px[i] = s_out[61] * (L.jtr[3 * j + c] - L.c[c]) + (c ? s_out[63] : s_out[62]);
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
        char who[48];
        snprintf(who, sizeof who, "dir_mano_para_smooth_step (hand %d)", s);
        if (int rc = dir::mano::check_mano_tables(t, who)) return rc;
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
