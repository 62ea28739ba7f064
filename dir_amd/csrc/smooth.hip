// Temporal smoothing of tracked predictions: the One-Euro filter (Casiez, Roussel, Vogel, CHI 2012) over every prediction stream of a
// batch of sequences, one launch per frame, with a jitter measure.  The reference has no temporal code; the rule is this project's own,
// written out in include/dir_hip.h and restated in float64 numpy by tests/helpers/one_euro_ref.py.
//
//   one_euro_kernel   one workgroup of 256 lanes per sequence (row).  Pass 1: every lane walks the row's F floats with stride 256 and the
//                     workgroup ORs "not finite".  Pass 2, per segment: lanes walk the segment's points with stride 256; a lane reads
//                     its point's D components of x and of the row's state, filters, writes y and shifts the history (a component is
//                     read and written by one lane only, so y may be x), and adds the point's second differences to its partial sums
//                     in point order.  The partials go through a fixed LDS tree and lane 0 adds them to the row's float64 accumulators.
//                     No atomics, no scratch, no workspace: a row's bits depend on nothing but the row.
#include <math.h>

#include "dir_common.h"

namespace {

constexpr int LANES = 256;
constexpr int AGE_MAX = 1 << 30;                          // `age` saturates here

struct Offsets {                                          // byte offsets inside one row of the state (dir_one_euro_state_bytes)
    long long jitter, y1, y2, x1, x2, dxhat, age, run, count, row;
};

bool layout(long long F, int S, Offsets& o) {
    if (F < 1 || F > DIR_ONE_EURO_MAX_VALUES || S < 1 || S > DIR_ONE_EURO_MAX_SEGMENTS) return false;
    o.jitter = 0;
    o.y1 = 16ll * S;
    o.y2 = o.y1 + 4 * F; o.x1 = o.y2 + 4 * F; o.x2 = o.x1 + 4 * F; o.dxhat = o.x2 + 4 * F;
    o.age = o.dxhat + 4 * F; o.run = o.age + 4; o.count = o.run + 4;
    o.row = (o.count + 4 + 15) / 16 * 16;
    return true;
}

struct Args {
    const float* x;
    const int* valid;
    float* y;
    int* updated;
    unsigned char* state;
    Offsets o;
    dir_one_euro_segment seg[DIR_ONE_EURO_MAX_SEGMENTS];
    int S, F, max_gap;
    double fps, d_cutoff;
    float min_cutoff, beta;
};

__device__ __forceinline__ float alpha(float r, float fc) {         // r = 2 pi dt
#pragma clang fp contract(off)
    return 1.f / (1.f + 1.f / (r * fc));
}

template <int D> __device__ __forceinline__ void walk_segment(const Args& a, int base, int n, float scale, int mode, float a_d, float r, float dt,
                                                             const float* x, float* y, float* y1, float* y2, float* x1, float* x2, float* dxhat,
                                                             bool jit, double& raw, double& fil) {
#pragma clang fp contract(off)
    for (int p = threadIdx.x; p < n; p += LANES) {
        const int at = base + p * D;
        float xv[D], yv[D], y1v[D], x1v[D];
#pragma unroll
        for (int c = 0; c < D; ++c) { xv[c] = x[at + c]; y1v[c] = y1[at + c]; x1v[c] = x1[at + c]; }
        if (mode == 2) {
#pragma unroll
            for (int c = 0; c < D; ++c) { yv[c] = xv[c]; dxhat[at + c] = 0.f; }
        } else {
            float v2 = 0.f, dh[D];
#pragma unroll
            for (int c = 0; c < D; ++c) {
                const float dx = (xv[c] - y1v[c]) / dt;
                const float h = dxhat[at + c];
                dh[c] = h + a_d * (dx - h);
                dxhat[at + c] = dh[c];
                v2 += dh[c] * dh[c];
            }
            const float fc = a.min_cutoff + a.beta * (scale * sqrtf(v2));
            const float al = alpha(r, fc);
#pragma unroll
            for (int c = 0; c < D; ++c) yv[c] = y1v[c] + al * (xv[c] - y1v[c]);
        }
        double r2 = 0., f2 = 0.;                          // the second differences in double: exact from the float32 values
#pragma unroll
        for (int c = 0; c < D; ++c) {
            const float x2v = x2[at + c], y2v = y2[at + c];
            const double dr = (double)xv[c] - 2. * (double)x1v[c] + (double)x2v, df = (double)yv[c] - 2. * (double)y1v[c] + (double)y2v;
            r2 += dr * dr; f2 += df * df;
            y[at + c] = yv[c];
            y2[at + c] = y1v[c]; y1[at + c] = yv[c];
            x2[at + c] = x1v[c]; x1[at + c] = xv[c];
        }
        if (jit) { raw += sqrt(r2); fil += sqrt(f2); }
    }
}

__global__ __launch_bounds__(LANES) void one_euro_kernel(Args a) {
#pragma clang fp contract(off)
    __shared__ double red[2][LANES];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* x = a.x + (long long)b * a.F;
    float* y = a.y + (long long)b * a.F;
    unsigned char* st = a.state + (long long)b * a.o.row;
    int* age_p = reinterpret_cast<int*>(st + a.o.age);
    int* run_p = reinterpret_cast<int*>(st + a.o.run);
    int* count_p = reinterpret_cast<int*>(st + a.o.count);

    int bad = a.valid && !a.valid[b];
    for (int i = tid; i < a.F; i += LANES) bad |= !isfinite(x[i]);
    bad = __syncthreads_or(bad);                          // also orders every read of x in this pass before any write of y below
    const int age = *age_p, run = *run_p;                 // read by every lane before lane 0 writes them, behind the barrier below
    __syncthreads();

    if (bad) {                                            // pass-through, bit for bit (NaN payloads included)
        const unsigned* xi = reinterpret_cast<const unsigned*>(x);
        unsigned* yi = reinterpret_cast<unsigned*>(y);
        for (int i = tid; i < a.F; i += LANES) yi[i] = xi[i];
        if (tid == 0) {
            if (age > 0) *age_p = age < AGE_MAX ? age + 1 : AGE_MAX;
            *run_p = 0;
            a.updated[b] = 0;
        }
        return;
    }
    const int mode = (age == 0 || age > a.max_gap) ? 2 : 1;
    const int run_new = mode == 2 ? 1 : (run < AGE_MAX ? run + 1 : AGE_MAX);
    const bool jit = run_new >= 3;
    const double dt = (double)age / a.fps;
    const float r = (float)(6.283185307179586476925286766559 * dt);
    const float a_d = (float)(1. / (1. + 1. / (6.283185307179586476925286766559 * a.d_cutoff * dt)));
    float* y1 = reinterpret_cast<float*>(st + a.o.y1);
    float* y2 = reinterpret_cast<float*>(st + a.o.y2);
    float* x1 = reinterpret_cast<float*>(st + a.o.x1);
    float* x2 = reinterpret_cast<float*>(st + a.o.x2);
    float* dxhat = reinterpret_cast<float*>(st + a.o.dxhat);
    double* acc = reinterpret_cast<double*>(st + a.o.jitter);

    int base = 0;
    for (int s = 0; s < a.S; ++s) {
        const int n = a.seg[s].n_points, D = a.seg[s].dims;
        const float scale = a.seg[s].speed_scale;
        double raw = 0., fil = 0.;
        switch (D) {
            case 1: walk_segment<1>(a, base, n, scale, mode, a_d, r, (float)dt, x, y, y1, y2, x1, x2, dxhat, jit, raw, fil); break;
            case 2: walk_segment<2>(a, base, n, scale, mode, a_d, r, (float)dt, x, y, y1, y2, x1, x2, dxhat, jit, raw, fil); break;
            case 3: walk_segment<3>(a, base, n, scale, mode, a_d, r, (float)dt, x, y, y1, y2, x1, x2, dxhat, jit, raw, fil); break;
            default: walk_segment<4>(a, base, n, scale, mode, a_d, r, (float)dt, x, y, y1, y2, x1, x2, dxhat, jit, raw, fil); break;
        }
        base += n * D;
        if (jit) {                                        // uniform over the workgroup
            red[0][tid] = raw; red[1][tid] = fil;
            __syncthreads();
            for (int o = LANES / 2; o > 0; o >>= 1) {
                if (tid < o) { red[0][tid] += red[0][tid + o]; red[1][tid] += red[1][tid + o]; }
                __syncthreads();
            }
            if (tid == 0) { acc[2 * s] += red[0][0]; acc[2 * s + 1] += red[1][0]; }
            __syncthreads();                              // red is written again by the next segment
        }
    }
    if (tid == 0) {
        *age_p = 1;
        *run_p = run_new;
        if (jit) *count_p += 1;
        a.updated[b] = mode;
    }
}

}  // namespace

extern "C" long long dir_one_euro_state_bytes(int F, int S, long long* offsets) {
    Offsets o;
    if (!layout(F, S, o)) return -1;
    if (offsets) {
        const long long v[9] = {o.jitter, o.y1, o.y2, o.x1, o.x2, o.dxhat, o.age, o.run, o.count};
        for (int i = 0; i < 9; ++i) offsets[i] = v[i];
    }
    return o.row;
}

extern "C" int dir_one_euro_step(const float* x, const int32_t* valid, int B, const dir_one_euro_segment* segments, int S, double fps,
                                 double min_cutoff, double beta, double d_cutoff, int max_gap, void* state, float* y, int32_t* updated,
                                 void* stream) {
    DIR_REQUIRE(x && segments && state && y && updated, "dir_one_euro_step: null pointer");
    DIR_REQUIRE(B >= 1 && B <= DIR_CROP_MAX_BATCH, "dir_one_euro_step: bad args (B %d outside 1..%d)", B, DIR_CROP_MAX_BATCH);
    DIR_REQUIRE(S >= 1 && S <= DIR_ONE_EURO_MAX_SEGMENTS, "dir_one_euro_step: bad args (%d segments outside 1..%d)", S, DIR_ONE_EURO_MAX_SEGMENTS);
    Args a;
    long long F = 0;
    for (int s = 0; s < S; ++s) {
        const dir_one_euro_segment& g = segments[s];
        DIR_REQUIRE(g.dims >= 1 && g.dims <= 4, "dir_one_euro_step: bad args (segment %d: D %d outside 1..4)", s, g.dims);
        DIR_REQUIRE(g.n_points >= 1 && g.n_points <= DIR_ONE_EURO_MAX_VALUES, "dir_one_euro_step: bad args (segment %d: %d points outside 1..%d)", s,
                    g.n_points, DIR_ONE_EURO_MAX_VALUES);
        DIR_REQUIRE(isfinite(g.speed_scale) && g.speed_scale >= 0.f, "dir_one_euro_step: bad args (segment %d: speed scale %g)", s, (double)g.speed_scale);
        F += (long long)g.n_points * g.dims;
        DIR_REQUIRE(F <= DIR_ONE_EURO_MAX_VALUES, "dir_one_euro_step: bad args (F %lld over the limit %d)", F, DIR_ONE_EURO_MAX_VALUES);
        a.seg[s] = g;
    }
    for (int s = S; s < DIR_ONE_EURO_MAX_SEGMENTS; ++s) a.seg[s] = dir_one_euro_segment{0, 1, 0.f};
    DIR_REQUIRE(isfinite(fps) && fps > 0. && isfinite(min_cutoff) && min_cutoff > 0. && isfinite(d_cutoff) && d_cutoff > 0. && isfinite(beta) &&
                    beta >= 0. && max_gap >= 1,
                "dir_one_euro_step: bad args (non-positive rate: fps %g, min_cutoff %g, d_cutoff %g must be > 0, beta %g >= 0, max_gap %d >= 1)", fps,
                min_cutoff, d_cutoff, beta, max_gap);
    DIR_REQUIRE(((uintptr_t)x & 3) == 0 && ((uintptr_t)y & 3) == 0 && ((uintptr_t)state & 7) == 0,
                "dir_one_euro_step: x and y must be 4-byte aligned, state 8-byte aligned");
    layout(F, S, a.o);
    a.x = x; a.valid = valid; a.y = y; a.updated = updated; a.state = static_cast<unsigned char*>(state);
    a.S = S; a.F = (int)F; a.max_gap = max_gap; a.fps = fps; a.d_cutoff = d_cutoff; a.min_cutoff = (float)min_cutoff; a.beta = (float)beta;
    DIR_LAUNCH(one_euro_kernel, dim3(B), dim3(LANES), 0, (hipStream_t)stream, a);
    return dir::check_launch("dir_one_euro_step");
}
