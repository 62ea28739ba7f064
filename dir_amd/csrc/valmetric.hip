// The per-epoch validation metric of the reference's training loop (InterHandDataset.evaluate, dataset/interhand.py:262-315, summed by
// Trainer.test_model, train.py:157-181) for every stage of one batch in one launch: MPJPE / MPVPE of both hands after root (MANO joint 9)
// and bone-length (|J9 - J0|) alignment.  One workgroup per sample stages the root-relative ground truth of both hands in LDS once
// (19 KB), walks the stages in the reference's fp32 operation order per point and sums the sample's norms in fp64; a one-workgroup tail
// adds the batch means to the caller's accumulator in a fixed order (no atomics: two calls on the same inputs give the same bits).
// HBM-bound: 19 KB of ground truth + 19 KB per stage and sample.
#include "dir_common.h"

namespace dir {
namespace {

constexpr int NV = 778, NJ = 21, VM_THREADS = 256, VM_WAVES = VM_THREADS / 64;

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ float norm3(float x, float y, float z) { return sqrtf(fmaf(z, z, fmaf(y, y, x * x))); }

// |J9 - J0| of one hand's [21,3] joints (interhand.py:270-271,283-284)
__device__ __forceinline__ float bone_length(const float* __restrict__ j) {
    return norm3(j[27] - j[0], j[28] - j[1], j[29] - j[2]);
}

__global__ __launch_bounds__(VM_THREADS) void val_metrics_kernel(dir_val_metrics_desc d, int n_stages, int B) {
    __shared__ float s_jg[2][NJ * 3], s_vg[2][NV * 3];        // ground truth minus its root (:272-273,301-302)
    __shared__ float s_len[2], s_root[2][3], s_scale[2];
    __shared__ double s_part[VM_WAVES][4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);

    if (tid < 2) s_len[tid] = bone_length(d.joints_gt[tid] + (size_t)b * NJ * 3);
    for (int h = 0; h < 2; ++h) {
        const float* jg = d.joints_gt[h] + (size_t)b * NJ * 3;
        const float* vg = d.verts_gt[h] + (size_t)b * NV * 3;
        const float r[3] = {jg[27], jg[28], jg[29]};
        for (int i = tid; i < NJ * 3; i += VM_THREADS) s_jg[h][i] = jg[i] - r[i % 3];
        for (int i = tid; i < NV * 3; i += VM_THREADS) s_vg[h][i] = vg[i] - r[i % 3];
    }
    __syncthreads();

    for (int s = 0; s < n_stages; ++s) {
        if (tid < 2) {                                        // :281-286: root and scale of the predicted hand
            const float* jp = d.joints_pd[s][tid] + (size_t)b * NJ * 3;
            s_root[tid][0] = jp[27], s_root[tid][1] = jp[28], s_root[tid][2] = jp[29];
            s_scale[tid] = s_len[tid] / bone_length(jp);
        }
        __syncthreads();
        double a[4] = {0, 0, 0, 0};                           // joint L, joint R, vert L, vert R
        for (int i = tid; i < 2 * (NJ + NV); i += VM_THREADS) {
            const int isv = i >= 2 * NJ, k2 = isv ? i - 2 * NJ : i, n = isv ? NV : NJ;
            const int h = k2 >= n, k = k2 - h * n;
            const float* p = (isv ? d.verts_pd[s][h] + (size_t)b * NV * 3 : d.joints_pd[s][h] + (size_t)b * NJ * 3) + k * 3;
            const float* g = (isv ? s_vg[h] : s_jg[h]) + k * 3;
            const float sc = s_scale[h];
            const float x = (p[0] - s_root[h][0]) * sc - g[0];      // :288-291,305-307: (pred - root) * scale - (gt - root)
            const float y = (p[1] - s_root[h][1]) * sc - g[1];
            const float z = (p[2] - s_root[h][2]) * sc - g[2];
            const double e = (double)norm3(x, y, z);
#pragma unroll
            for (int q = 0; q < 4; ++q) a[q] += (q == 2 * isv + h) ? e : 0.0;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) a[q] = wave_sum_d(a[q]);
        if (lane == 0) {
#pragma unroll
            for (int q = 0; q < 4; ++q) s_part[wave][q] = a[q];
        }
        __syncthreads();
        if (tid < 4) {
            double t = 0;
            for (int w = 0; w < VM_WAVES; ++w) t += s_part[w][tid];
            d.sample_sums[((size_t)s * B + b) * 4 + tid] = t;
        }
        __syncthreads();                                      // s_root / s_scale / s_part are rewritten by the next stage
    }
}

// batch means (:292-310: mean over (B, 21) resp. (B, 778), * 1000) added to the running sums of train.py:167-170; one thread per
// (stage, quantity) walks the samples in order
__global__ __launch_bounds__(64) void val_metrics_accumulate_kernel(dir_val_metrics_desc d, int n_stages, int B) {
    const int t = threadIdx.x;
    if (t < n_stages * 4) {
        const int s = t >> 2, q = t & 3;
        double sum = 0;
        for (int b = 0; b < B; ++b) sum += d.sample_sums[((size_t)s * B + b) * 4 + q];
        d.acc[t] += sum / ((double)B * (q < 2 ? NJ : NV)) * 1000.0;
    }
    if (t == 0) *d.batches += 1;                              // train.py:174
}

}  // namespace
}  // namespace dir

extern "C" int dir_val_metrics_forward(const dir_val_metrics_desc* desc, int n_stages, int B, void* stream) {
    DIR_REQUIRE(desc, "dir_val_metrics_forward: null descriptor");
    DIR_REQUIRE(B >= 0, "dir_val_metrics_forward: B=%d", B);
    DIR_REQUIRE(n_stages >= 1 && n_stages <= DIR_VAL_MAX_STAGES, "dir_val_metrics_forward: n_stages=%d not in 1..%d", n_stages,
                DIR_VAL_MAX_STAGES);
    for (int h = 0; h < 2; ++h) {
        DIR_REQUIRE(desc->joints_gt[h] && desc->verts_gt[h], "dir_val_metrics_forward: null pointer (ground truth, hand %d)", h);
        for (int s = 0; s < n_stages; ++s)
            DIR_REQUIRE(desc->joints_pd[s][h] && desc->verts_pd[s][h], "dir_val_metrics_forward: null pointer (stage %d, hand %d)", s, h);
    }
    DIR_REQUIRE(desc->sample_sums && desc->acc && desc->batches, "dir_val_metrics_forward: null pointer (sample_sums / acc / batches)");
    if (B == 0) return DIR_OK;
    DIR_LAUNCH(dir::val_metrics_kernel, dim3(B), dim3(dir::VM_THREADS), 0, (hipStream_t)stream, *desc, n_stages, B);
    if (int rc = dir::check_launch("dir_val_metrics_forward")) return rc;
    DIR_LAUNCH(dir::val_metrics_accumulate_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, *desc, n_stages, B);
    return dir::check_launch("dir_val_metrics_forward (accumulate)");
}
