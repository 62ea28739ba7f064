// Aligned evaluation measures: the similarity (Procrustes) fit of a predicted point set onto its ground truth, nearest-neighbour
// distances between two point sets, and pooled threshold counts (PCK curves).  The rules, which tests/helpers/alignment_ref.py restates
// in float64:
//
//   fit         p = pd - mean(pd), g = gt - mean(gt) (the means as first point + mean of the differences from it); R = the PROPER rotation that maximises sum g_i . R p_i;
//               s = sum g_i . R p_i / sum |p_i|^2 (1 without DIR_ALIGN_SCALE); t = mean(gt) - s R mean(pd); aligned = s R pd + t,
//               evaluated as s R p + mean(gt); err = |aligned - gt|
//   rotation    Horn 1987: with S[a][b] = sum p_a g_b, the unit quaternion q that maximises q^T N q for the symmetric 4 x 4
//               N = [[Sxx+Syy+Szz, Syz-Szy, Szx-Sxz, Sxy-Syx], [., Sxx-Syy-Szz, Sxy+Syx, Szx+Sxz], [., ., -Sxx+Syy-Szz, Syz+Szy],
//               [., ., ., -Sxx-Syy+Szz]], found by cyclic Jacobi sweeps on N / max|N| (horn_rotation.h, shared with mano_fit_start.hip).  A unit quaternion is a rotation, never a reflection,
//               and nothing is squared on the way: a planar set keeps its third singular value's sign information.
//   invalid     a sample with a non-finite coordinate or sum |p_i|^2 = 0: NaN in all of its outputs
//   nn          d_ab[i] = min_j |a_i - b_j|, point to point, the differences taken before squaring (identical sets give exactly 0);
//               non-finite target points are passed over, a non-finite query point gives NaN
//   counts      counts[k] += #{finite err <= thresholds[k]}, counts[K] += #{finite err}
//
//   procrustes_kernel   one workgroup per sample.  Two passes over the sample (means; then the nine sums of S and sum |p|^2 about the
//                       means), each thread adding its points in index order, then a fixed xor tree over the wave and the waves in order:
//                       the block size depends on N only, so a sample's sums are the same bits in any batch.  Thread 0 solves the 4 x 4
//                       eigenproblem in registers (every index a compile-time constant); a third pass writes aligned / err.
//   nn_kernel           one workgroup per (sample, direction).  The target set is staged in LDS (PC points per chunk) and every lane walks
//                       it in index order for its own points: all lanes read the same LDS address, a broadcast.
//   counts_kernel       every wave holds VPT values per lane and walks the thresholds (staged in LDS): one ballot + popcount per value
//                       and threshold, added to the wave's own LDS row; the rows leave the workgroup as integer atomics.
//
// float32 throughout, no floating-point atomics; integer sums do not depend on the order.
#include "horn_rotation.h"

namespace {

using dir::horn_rotation;

constexpr int PT = 256;                // procrustes_kernel: threads at most
constexpr int NRED = 10;               // values reduced per pass at most
constexpr int PC = 2048;               // nn_kernel: target points per LDS chunk (float4 each)
constexpr int QPT = DIR_MESH_MAX_VERTS / 1024;      // query points per thread at most
constexpr int CT = 256, VPT = 4;       // counts_kernel: threads per workgroup, values per lane and pass

__device__ __forceinline__ bool finite3(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }

// block sum of K values per thread in a fixed order: xor tree over each wave, then the waves in order; every thread gets the result
template <int K> __device__ __forceinline__ void block_sum(float (&v)[K], float (*part)[NRED], int tid, int T) {
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = dir::wave_sum(v[k]);
    __syncthreads();                   // the previous use of `part` is over
    if ((tid & 63) == 0)
#pragma unroll
        for (int k = 0; k < K; ++k) part[tid >> 6][k] = v[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        float s = part[0][k];
        for (int w = 1; w < (T >> 6); ++w) s += part[w][k];
        v[k] = s;
    }
}

__global__ __launch_bounds__(PT) void procrustes_kernel(const float* __restrict__ pd, const float* __restrict__ gt, int N, int flags,
                                                        float* __restrict__ transform, float* __restrict__ aligned,
                                                        float* __restrict__ err) {
    __shared__ float part[PT / 64][NRED];
    __shared__ float sol[16];          // s, R, and 1 = the sample is valid
    const int b = blockIdx.x, tid = threadIdx.x, T = blockDim.x;
    const float* P = pd + (long long)b * N * 3;
    const float* G = gt + (long long)b * N * 3;
    // pass 1: the means, taken about the sample's first point: a set of equal points has exactly that point as its mean, so sum |p|^2 is
    // exactly 0 for it, whatever the coordinates are
    const float o[6] = {P[0], P[1], P[2], G[0], G[1], G[2]};
    float m[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    bool bad = false;
    for (int i = tid; i < N; i += T) {
        const float px = P[3 * i], py = P[3 * i + 1], pz = P[3 * i + 2], gx = G[3 * i], gy = G[3 * i + 1], gz = G[3 * i + 2];
        bad |= !(finite3(px, py, pz) && finite3(gx, gy, gz));
        m[0] += px - o[0], m[1] += py - o[1], m[2] += pz - o[2], m[3] += gx - o[3], m[4] += gy - o[4], m[5] += gz - o[5];
    }
    block_sum<6>(m, part, tid, T);
    const float inv_n = 1.f / (float)N;
#pragma unroll
    for (int k = 0; k < 6; ++k) m[k] = o[k] + m[k] * inv_n;
    // pass 2: S[a][b] = sum p_a g_b and sum |p|^2, about the means
    float r[NRED] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int i = tid; i < N; i += T) {
        const float px = P[3 * i] - m[0], py = P[3 * i + 1] - m[1], pz = P[3 * i + 2] - m[2];
        const float gx = G[3 * i] - m[3], gy = G[3 * i + 1] - m[4], gz = G[3 * i + 2] - m[5];
        r[0] += px * gx, r[1] += px * gy, r[2] += px * gz;
        r[3] += py * gx, r[4] += py * gy, r[5] += py * gz;
        r[6] += pz * gx, r[7] += pz * gy, r[8] += pz * gz;
        r[9] += px * px + py * py + pz * pz;
    }
    block_sum<NRED>(r, part, tid, T);
    bad = __syncthreads_or(bad);
    if (tid == 0) {
        float S[9], R[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 9; ++k) S[k] = r[k];
        const bool ok = !bad && r[9] > 0.f && isfinite(r[9]);
        float s = 1.f;
        if (ok) {
            horn_rotation(S, R);
            // sum g . R p = sum_ab R[a][b] S[b][a]
            const float num = R[0] * S[0] + R[1] * S[3] + R[2] * S[6] + R[3] * S[1] + R[4] * S[4] + R[5] * S[7] + R[6] * S[2] + R[7] * S[5] + R[8] * S[8];
            if (flags & DIR_ALIGN_SCALE) s = num / r[9];
        }
        sol[0] = s;
#pragma unroll
        for (int k = 0; k < 9; ++k) sol[1 + k] = ok ? R[k] : 0.f;
        sol[10] = ok && isfinite(s) ? 1.f : 0.f;
    }
    __syncthreads();
    const float qnan = __builtin_nanf("");
    const bool ok = sol[10] != 0.f;
    const float s = sol[0];
    float R[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = sol[1 + k];
    if (transform && tid < 13) {
        float val = qnan;
        if (ok) {
            if (tid < 10) val = sol[tid];          // s, then R
            else {
                const int a = tid - 10;          // t = mean(gt) - s R mean(pd)
                val = m[3 + a] - s * (sol[1 + 3 * a] * m[0] + sol[2 + 3 * a] * m[1] + sol[3 + 3 * a] * m[2]);
            }
        }
        transform[(long long)b * 13 + tid] = val;
    }
    // pass 3: aligned = s R p + mean(gt) and the distances
    for (int i = tid; i < N; i += T) {
        const float px = P[3 * i] - m[0], py = P[3 * i + 1] - m[1], pz = P[3 * i + 2] - m[2];
        float ax = s * (R[0] * px + R[1] * py + R[2] * pz) + m[3];
        float ay = s * (R[3] * px + R[4] * py + R[5] * pz) + m[4];
        float az = s * (R[6] * px + R[7] * py + R[8] * pz) + m[5];
        const float dx = ax - G[3 * i], dy = ay - G[3 * i + 1], dz = az - G[3 * i + 2];
        float e = sqrtf(dx * dx + dy * dy + dz * dz);
        if (!ok) ax = ay = az = e = qnan;
        const long long at = (long long)b * N + i;
        if (aligned) aligned[3 * at] = ax, aligned[3 * at + 1] = ay, aligned[3 * at + 2] = az;
        err[at] = e;
    }
}

__global__ __launch_bounds__(1024) void nn_kernel(const float* __restrict__ a, const float* __restrict__ b, int Na, int Nb,
                                                  float* __restrict__ d_ab, float* __restrict__ d_ba) {
    __shared__ float4 pts[PC];
    const int s = blockIdx.x >> 1, dir = blockIdx.x & 1, tid = threadIdx.x, T = blockDim.x;
    // direction 0: a's points against the set b; direction 1: b's points against the set a
    const int Nq = dir ? Nb : Na, Nt = dir ? Na : Nb;
    const float* q = dir ? b + (long long)s * Nb * 3 : a + (long long)s * Na * 3;
    const float* t = dir ? a + (long long)s * Na * 3 : b + (long long)s * Nb * 3;
    float* out = dir ? d_ba + (long long)s * Nb : d_ab + (long long)s * Na;
    float px[QPT], py[QPT], pz[QPT], d2[QPT];
#pragma unroll
    for (int k = 0; k < QPT; ++k) {
        const int v = tid + k * T;
        px[k] = v < Nq ? q[3 * v] : 0.f, py[k] = v < Nq ? q[3 * v + 1] : 0.f, pz[k] = v < Nq ? q[3 * v + 2] : 0.f;
        d2[k] = INFINITY;
    }
    for (int c0 = 0; c0 < Nt; c0 += PC) {
        const int n = min(PC, Nt - c0);
        __syncthreads();
        for (int i = tid; i < n; i += T) pts[i] = make_float4(t[3 * (c0 + i)], t[3 * (c0 + i) + 1], t[3 * (c0 + i) + 2], 0.f);
        __syncthreads();
#pragma unroll
        for (int k = 0; k < QPT; ++k) {
            if (tid + k * T >= Nq) continue;
            float best = d2[k];
            for (int j = 0; j < n; ++j) {
                const float4 p = pts[j];
                const float dx = p.x - px[k], dy = p.y - py[k], dz = p.z - pz[k];
                best = fminf(best, dx * dx + dy * dy + dz * dz);          // a NaN (non-finite target point) is passed over
            }
            d2[k] = best;
        }
    }
#pragma unroll
    for (int k = 0; k < QPT; ++k) {
        const int v = tid + k * T;
        if (v < Nq) out[v] = finite3(px[k], py[k], pz[k]) ? sqrtf(d2[k]) : __builtin_nanf("");
    }
}

__global__ __launch_bounds__(CT) void counts_kernel(const float* __restrict__ err, long long n, const float* __restrict__ thresholds, int K,
                                                    unsigned long long* __restrict__ counts) {
    extern __shared__ float dyn[];     // thresholds [K], then one row of K + 1 counts per wave
    float* thr = dyn;
    int* rows = reinterpret_cast<int*>(dyn + K);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (int k = tid; k < K; k += CT) thr[k] = thresholds[k];
    for (int k = tid; k < (CT / 64) * (K + 1); k += CT) rows[k] = 0;
    __syncthreads();
    int* row = rows + wave * (K + 1);
    const long long per_pass = (long long)CT * VPT;
    for (long long base = (long long)blockIdx.x * per_pass; base < n; base += (long long)gridDim.x * per_pass) {
        float v[VPT];
        int nfin = 0;
#pragma unroll
        for (int u = 0; u < VPT; ++u) {
            const long long i = base + u * CT + tid;
            const float e = i < n ? err[i] : INFINITY;
            v[u] = isfinite(e) ? e : __builtin_nanf("");          // a NaN compares false with every threshold
            nfin += __popcll(__ballot(isfinite(e)));
        }
        for (int k = 0; k < K; ++k) {
            const float t = thr[k];
            int c = 0;
#pragma unroll
            for (int u = 0; u < VPT; ++u) c += __popcll(__ballot(v[u] <= t));
            if (lane == 0) row[k] += c;          // the wave's own row: no other wave touches it
        }
        if (lane == 0) row[K] += nfin;
    }
    __syncthreads();
    for (int k = tid; k <= K; k += CT) {
        int c = 0;
#pragma unroll
        for (int w = 0; w < CT / 64; ++w) c += rows[w * (K + 1) + k];
        if (c) atomicAdd(counts + k, (unsigned long long)c);          // integers: the total does not depend on the order
    }
}

}  // namespace

extern "C" int dir_procrustes_align(const float* pd, const float* gt, int B, int N, int flags, float* transform, float* aligned, float* err,
                                    void* stream) {
    DIR_REQUIRE(pd && gt && err, "dir_procrustes_align: null pointer (pd / gt / err)");
    DIR_REQUIRE(B > 0 && B <= DIR_MESH_MAX_BATCH, "dir_procrustes_align: batch %d outside 1..%d", B, DIR_MESH_MAX_BATCH);
    DIR_REQUIRE(N >= 3 && N <= DIR_MESH_MAX_VERTS, "dir_procrustes_align: %d points outside 3..%d", N, DIR_MESH_MAX_VERTS);
    DIR_REQUIRE((flags & ~DIR_ALIGN_SCALE) == 0, "dir_procrustes_align: unknown flags 0x%x", flags);
    // whole waves, as many as the points fill, 256 threads at most: a function of N alone, so a sample's sums are the same in any batch
    const int T = N >= PT ? PT : (N + 63) / 64 * 64;
    DIR_LAUNCH(procrustes_kernel, dim3(B), dim3(T), 0, (hipStream_t)stream, pd, gt, N, flags, transform, aligned, err);
    return dir::check_launch("dir_procrustes_align");
}

extern "C" int dir_point_set_nn(const float* a, const float* b, int B, int Na, int Nb, float* d_ab, float* d_ba, void* stream) {
    DIR_REQUIRE(a && b && d_ab && d_ba, "dir_point_set_nn: null pointer");
    DIR_REQUIRE(B > 0 && B <= DIR_MESH_MAX_BATCH, "dir_point_set_nn: batch %d outside 1..%d", B, DIR_MESH_MAX_BATCH);
    DIR_REQUIRE(Na > 0 && Nb > 0 && Na <= DIR_MESH_MAX_VERTS && Nb <= DIR_MESH_MAX_VERTS, "dir_point_set_nn: %d / %d points outside 1..%d", Na,
                Nb, DIR_MESH_MAX_VERTS);
    // as few passes over the query points as 1024 threads allow, in whole waves (778 points on 832 threads)
    const int nq = Na > Nb ? Na : Nb, passes = (nq + 1023) / 1024, T = ((nq + passes - 1) / passes + 63) / 64 * 64;
    DIR_LAUNCH(nn_kernel, dim3(2 * B), dim3(T), 0, (hipStream_t)stream, a, b, Na, Nb, d_ab, d_ba);
    return dir::check_launch("dir_point_set_nn");
}

extern "C" int dir_threshold_counts(const float* err, long long n, const float* thresholds, int K, long long* counts, void* stream) {
    DIR_REQUIRE(err && thresholds && counts, "dir_threshold_counts: null pointer");
    DIR_REQUIRE(n > 0 && n <= DIR_ALIGN_MAX_VALUES, "dir_threshold_counts: %lld values outside 1..%lld", n, (long long)DIR_ALIGN_MAX_VALUES);
    DIR_REQUIRE(K > 0 && K <= DIR_ALIGN_MAX_THRESHOLDS, "dir_threshold_counts: %d thresholds outside 1..%d", K, DIR_ALIGN_MAX_THRESHOLDS);
    const long long per_pass = (long long)CT * VPT, want = (n + per_pass - 1) / per_pass;
    const int grid = (int)(want < 1024 ? want : 1024);
    const size_t lds = sizeof(float) * K + sizeof(int) * (CT / 64) * (K + 1);
    DIR_LAUNCH(counts_kernel, dim3(grid), dim3(CT), lds, (hipStream_t)stream, err, n, thresholds, K, reinterpret_cast<unsigned long long*>(counts));
    return dir::check_launch("dir_threshold_counts");
}
