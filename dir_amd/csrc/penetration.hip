// Inter-hand penetration of two batched triangle meshes (the ObMan measures of Hasson et al. 2019: penetration depth and intersection
// volume).  Both are queries of many points against a mesh; the rules, which tests/helpers/penetration_ref.py restates in float64:
//
//   skipped     a face with a repeated vertex index or an index outside 0..V-1 takes part in nothing
//   winding     w(p) = (1/4 pi) sum_f 2 atan2(det[a b c], |a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b|), a, b, c the face's corners minus p
//               (Van Oosterom-Strackee); atan2(0, 0) counts as 0.  The terms are added in face order, one accumulator per point.
//   inside      |w(p)| > 0.5: independent of the face orientation, tolerant of an open boundary (MANO's wrist)
//   distance    d(p) = min over the faces of the distance to the closest point of the closed triangle (Ericson, Real-Time Collision
//               Detection 5.1.5, with p at the origin; a zero denominator, which only a degenerate triangle gives, takes parameter 0)
//   lattice     points (i h, j h, k h), evaluated as float(i) * h, i in ceil(lo / h) .. floor(hi / h) per axis, lo = max(min_a, min_b),
//               hi = min(max_a, max_b) over ALL vertices of each mesh (correctly rounded float32 division)
//
//   penetration_kernel  one workgroup per (sample, direction).  The target mesh's corner triples are staged in LDS (FC faces per
//                       chunk; MANO's 1 538 are one chunk) and every lane owns query vertices, walking the staged faces in index
//                       order: all lanes read the same LDS address (a broadcast, conflict-free) and each point's sum has one fixed
//                       order whatever the batch size is.  count / max / sum over the inside vertices: per thread in vertex order,
//                       then a fixed xor tree over the wave and the waves in order.  The block size depends on the mesh sizes only.
//   volume_kernel       VG workgroups per sample, one lattice point per lane.  Every workgroup derives the lattice from the two
//                       bounding boxes itself (min / max are exact, so all agree), so no host read sizes anything.  Mesh A is staged
//                       and tested first; mesh B is staged only when some point of the workgroup is inside A, and walked only by
//                       those lanes.  The count goes out with one integer atomic per workgroup; volume_finish_kernel writes the volume.
//
// float32 throughout, no floating-point atomics; the results do not depend on the schedule.
#include "dir_common.h"

namespace {

constexpr int FC = 1600;               // faces per LDS chunk
constexpr int TS = 10;                 // dwords per staged face: nine corner coordinates and the valid flag
constexpr int QPT = DIR_MESH_MAX_VERTS / 1024;      // query vertices per thread at most
constexpr int VT = 256, VG = 16;       // volume_kernel: threads per workgroup, workgroups per sample
constexpr float INV_2PI = 0.15915494309189535f;

// faces f0 .. f0 + n - 1 of one sample's mesh into LDS
__device__ __forceinline__ void stage_faces(float* tri, const float* verts, const int32_t* faces, int V, int f0, int n, int tid, int T) {
    for (int i = tid; i < n; i += T) {
        const int32_t* fp = faces + 3 * (long long)(f0 + i);
        const int ia = fp[0], ib = fp[1], ic = fp[2];
        const bool ok = (unsigned)ia < (unsigned)V && (unsigned)ib < (unsigned)V && (unsigned)ic < (unsigned)V && ia != ib && ib != ic && ia != ic;
        float* t = tri + i * TS;
        const int id[3] = {ia, ib, ic};
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int k = 0; k < 3; ++k) t[3 * c + k] = ok ? verts[3 * id[c] + k] : 0.f;
        t[9] = ok ? 1.f : 0.f;
    }
}

__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) { return ax * bx + ay * by + az * bz; }
__device__ __forceinline__ float ratio(float n, float d) { return d != 0.f ? n / d : 0.f; }

// squared distance from the origin to the closed triangle (a, b, c)
__device__ __forceinline__ float tri_dist2(float ax, float ay, float az, float bx, float by, float bz, float cx, float cy, float cz) {
    const float ux = bx - ax, uy = by - ay, uz = bz - az, vx = cx - ax, vy = cy - ay, vz = cz - az;
    const float d1 = -dot3(ux, uy, uz, ax, ay, az), d2 = -dot3(vx, vy, vz, ax, ay, az);
    if (d1 <= 0.f && d2 <= 0.f) return dot3(ax, ay, az, ax, ay, az);
    const float d3 = -dot3(ux, uy, uz, bx, by, bz), d4 = -dot3(vx, vy, vz, bx, by, bz);
    if (d3 >= 0.f && d4 <= d3) return dot3(bx, by, bz, bx, by, bz);
    const float d5 = -dot3(ux, uy, uz, cx, cy, cz), d6 = -dot3(vx, vy, vz, cx, cy, cz);
    if (d6 >= 0.f && d5 <= d6) return dot3(cx, cy, cz, cx, cy, cz);
    const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    float qx, qy, qz;
    if (vc <= 0.f && d1 >= 0.f && d3 <= 0.f) {
        const float t = ratio(d1, d1 - d3);
        qx = ax + t * ux, qy = ay + t * uy, qz = az + t * uz;
    } else if (vb <= 0.f && d2 >= 0.f && d6 <= 0.f) {
        const float t = ratio(d2, d2 - d6);
        qx = ax + t * vx, qy = ay + t * vy, qz = az + t * vz;
    } else if (va <= 0.f && d4 - d3 >= 0.f && d5 - d6 >= 0.f) {
        const float t = ratio(d4 - d3, (d4 - d3) + (d5 - d6));
        qx = bx + t * (cx - bx), qy = by + t * (cy - by), qz = bz + t * (cz - bz);
    } else {
        const float s = va + vb + vc, v = ratio(vb, s), w = ratio(vc, s);
        qx = ax + ux * v + vx * w, qy = ay + uy * v + vy * w, qz = az + uz * v + vz * w;
    }
    return dot3(qx, qy, qz, qx, qy, qz);
}

// n staged faces against the point p: adds the atan2 terms to `acc` (the winding number is acc / 2 pi) and lowers `dmin2`
template <bool DIST> __device__ __forceinline__ void walk_faces(const float* tri, int n, float px, float py, float pz, float& acc, float& dmin2) {
    for (int f = 0; f < n; ++f) {
        const float* t = tri + f * TS;
        if (t[9] == 0.f) continue;          // the same for every lane
        const float ax = t[0] - px, ay = t[1] - py, az = t[2] - pz, bx = t[3] - px, by = t[4] - py, bz = t[5] - pz;
        const float cx = t[6] - px, cy = t[7] - py, cz = t[8] - pz;
        const float la = sqrtf(dot3(ax, ay, az, ax, ay, az)), lb = sqrtf(dot3(bx, by, bz, bx, by, bz)), lc = sqrtf(dot3(cx, cy, cz, cx, cy, cz));
        const float det = ax * (by * cz - bz * cy) + ay * (bz * cx - bx * cz) + az * (bx * cy - by * cx);
        const float den = la * lb * lc + dot3(ax, ay, az, bx, by, bz) * lc + dot3(bx, by, bz, cx, cy, cz) * la + dot3(cx, cy, cz, ax, ay, az) * lb;
        acc += (det == 0.f && den == 0.f) ? 0.f : atan2f(det, den);
        if (DIST) dmin2 = fminf(dmin2, tri_dist2(ax, ay, az, bx, by, bz, cx, cy, cz));
    }
}

__global__ __launch_bounds__(1024) void penetration_kernel(const float* __restrict__ verts_a, const int32_t* __restrict__ faces_a,
                                                           const float* __restrict__ verts_b, const int32_t* __restrict__ faces_b, int Va, int Fa,
                                                           int Vb, int Fb, float* __restrict__ winding, float* __restrict__ dist,
                                                           int32_t* __restrict__ count, float* __restrict__ max_depth, float* __restrict__ sum_depth) {
    __shared__ float tri[FC * TS];
    const int b = blockIdx.x >> 1, dir = blockIdx.x & 1, tid = threadIdx.x, T = blockDim.x;
    // direction 0: A's vertices against mesh B; direction 1: B's vertices against mesh A
    const int Vq = dir ? Vb : Va, Vt = dir ? Va : Vb, Ft = dir ? Fa : Fb;
    const float* q = dir ? verts_b + (long long)b * Vb * 3 : verts_a + (long long)b * Va * 3;
    const float* tv = dir ? verts_a + (long long)b * Va * 3 : verts_b + (long long)b * Vb * 3;
    const int32_t* tf = dir ? faces_a : faces_b;
    float px[QPT], py[QPT], pz[QPT], acc[QPT], d2[QPT];
#pragma unroll
    for (int k = 0; k < QPT; ++k) {
        const int v = tid + k * T;
        px[k] = v < Vq ? q[3 * v] : 0.f, py[k] = v < Vq ? q[3 * v + 1] : 0.f, pz[k] = v < Vq ? q[3 * v + 2] : 0.f;
        acc[k] = 0.f, d2[k] = INFINITY;
    }
    for (int f0 = 0; f0 < Ft; f0 += FC) {
        const int n = min(FC, Ft - f0);
        __syncthreads();
        stage_faces(tri, tv, tf, Vt, f0, n, tid, T);
        __syncthreads();
#pragma unroll
        for (int k = 0; k < QPT; ++k)
            if (tid + k * T < Vq) walk_faces<true>(tri, n, px[k], py[k], pz[k], acc[k], d2[k]);
    }
    int cnt = 0;
    float mx = 0.f, sm = 0.f;
    const long long row = (long long)b * (Va + Vb) + (dir ? Va : 0);
#pragma unroll
    for (int k = 0; k < QPT; ++k) {
        const int v = tid + k * T;
        if (v >= Vq) continue;
        const float w = acc[k] * INV_2PI, d = sqrtf(d2[k]);
        if (winding) winding[row + v] = w;
        if (dist) dist[row + v] = d;
        if (fabsf(w) > 0.5f) cnt += 1, mx = fmaxf(mx, d), sm += d;
    }
    // the block's aggregate: a fixed xor tree over each wave, then the waves in order
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    mx = dir::wave_max(mx);
    sm = dir::wave_sum(sm);
    __syncthreads();                     // every wave is done with the staged faces
    const int wave = tid >> 6, nw = T >> 6;
    if ((tid & 63) == 0) tri[3 * wave] = __int_as_float(cnt), tri[3 * wave + 1] = mx, tri[3 * wave + 2] = sm;
    __syncthreads();
    if (tid == 0) {
        cnt = 0, mx = 0.f, sm = 0.f;
        for (int w = 0; w < nw; ++w) cnt += __float_as_int(tri[3 * w]), mx = fmaxf(mx, tri[3 * w + 1]), sm += tri[3 * w + 2];
        count[2 * b + dir] = cnt, max_depth[2 * b + dir] = mx, sum_depth[2 * b + dir] = sm;
    }
}

__global__ __launch_bounds__(VT) void volume_kernel(const float* __restrict__ verts_a, const int32_t* __restrict__ faces_a,
                                                    const float* __restrict__ verts_b, const int32_t* __restrict__ faces_b, int Va, int Fa, int Vb,
                                                    int Fb, float h, int max_cells, int32_t* __restrict__ n_both, int32_t* __restrict__ cells) {
    __shared__ float tri[FC * TS];
    __shared__ float box[VT / 64][12];
    __shared__ int part[VT / 64];
    const int b = blockIdx.x / VG, g = blockIdx.x % VG, tid = threadIdx.x;
    const float* va = verts_a + (long long)b * Va * 3;
    const float* vb = verts_b + (long long)b * Vb * 3;
    // r[0..2] = -min_a, r[3..5] = max_a, r[6..8] = -min_b, r[9..11] = max_b: one max reduction (min and max are exact in any order)
    float r[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) r[k] = -INFINITY;
    for (int v = tid; v < Va; v += VT)
#pragma unroll
        for (int k = 0; k < 3; ++k) r[k] = fmaxf(r[k], -va[3 * v + k]), r[3 + k] = fmaxf(r[3 + k], va[3 * v + k]);
    for (int v = tid; v < Vb; v += VT)
#pragma unroll
        for (int k = 0; k < 3; ++k) r[6 + k] = fmaxf(r[6 + k], -vb[3 * v + k]), r[9 + k] = fmaxf(r[9 + k], vb[3 * v + k]);
#pragma unroll
    for (int k = 0; k < 12; ++k) r[k] = dir::wave_max(r[k]);
    if ((tid & 63) == 0)
#pragma unroll
        for (int k = 0; k < 12; ++k) box[tid >> 6][k] = r[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 12; ++k) r[k] = fmaxf(fmaxf(box[0][k], box[1][k]), fmaxf(box[2][k], box[3][k]));
    static_assert(VT == 256, "four waves are combined above");
    // the lattice of the boxes' intersection; an index beyond 2^24 (float(i) is no longer every integer) counts as too many cells
    int i0[3] = {0, 0, 0}, nn[3] = {1, 1, 1};
    bool empty = false, over = false;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float lo = fmaxf(-r[k], -r[6 + k]), hi = fminf(r[3 + k], r[9 + k]);
        const float c0 = ceilf(lo / h), c1 = floorf(hi / h);
        if (!(c0 <= c1)) empty = true;          // disjoint boxes, or a box without a finite vertex
        else if (fabsf(c0) > 16777216.f || fabsf(c1) > 16777216.f || c1 - c0 + 1.f > (float)max_cells) over = true;
        else i0[k] = (int)c0, nn[k] = (int)c1 - (int)c0 + 1;
    }
    long long cells_ll = (long long)nn[0] * nn[1];          // each factor is at most max_cells <= 2^24
    cells_ll = cells_ll > max_cells ? (long long)max_cells + 1 : cells_ll * nn[2];
    const int total = empty ? 0 : (over || cells_ll > max_cells) ? max_cells + 1 : (int)cells_ll;
    if (g == 0 && tid == 0) cells[b] = total;
    if (total > max_cells || total == 0) return;
    int cnt = 0;
    for (int base = g * VT; base < total; base += VG * VT) {
        const int idx = base + tid;
        const bool active = idx < total;
        const int kz = idx % nn[2], jy = (idx / nn[2]) % nn[1], ix = idx / (nn[2] * nn[1]);
        const float px = (float)(i0[0] + ix) * h, py = (float)(i0[1] + jy) * h, pz = (float)(i0[2] + kz) * h;
        float acc = 0.f, unused = 0.f;
        for (int f0 = 0; f0 < Fa; f0 += FC) {
            const int n = min(FC, Fa - f0);
            __syncthreads();
            stage_faces(tri, va, faces_a, Va, f0, n, tid, VT);
            __syncthreads();
            if (active) walk_faces<false>(tri, n, px, py, pz, acc, unused);
        }
        const bool in_a = active && fabsf(acc * INV_2PI) > 0.5f;
        if (!__syncthreads_or(in_a)) continue;
        acc = 0.f;
        for (int f0 = 0; f0 < Fb; f0 += FC) {
            const int n = min(FC, Fb - f0);
            __syncthreads();
            stage_faces(tri, vb, faces_b, Vb, f0, n, tid, VT);
            __syncthreads();
            if (in_a) walk_faces<false>(tri, n, px, py, pz, acc, unused);
        }
        cnt += (in_a && fabsf(acc * INV_2PI) > 0.5f) ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if ((tid & 63) == 0) part[tid >> 6] = cnt;
    __syncthreads();
    if (tid == 0) {
        cnt = part[0] + part[1] + part[2] + part[3];
        if (cnt) atomicAdd(n_both + b, cnt);          // integers: the total does not depend on the order
    }
}

__global__ void volume_finish_kernel(const int32_t* __restrict__ n_both, const int32_t* __restrict__ cells, float h, int max_cells, int B,
                                     float* __restrict__ volume) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) volume[b] = cells[b] > max_cells ? __builtin_nanf("") : (float)n_both[b] * (h * h * h);
}

int check_meshes(const char* what, const void* verts_a, const void* faces_a, const void* verts_b, const void* faces_b, int B, int Va, int Fa,
                 int Vb, int Fb) {
    DIR_REQUIRE(verts_a && faces_a && verts_b && faces_b, "%s: null pointer", what);
    DIR_REQUIRE(B > 0 && B <= DIR_MESH_MAX_BATCH, "%s: batch %d outside 1..%d", what, B, DIR_MESH_MAX_BATCH);
    DIR_REQUIRE(Va > 0 && Vb > 0 && Va <= DIR_MESH_MAX_VERTS && Vb <= DIR_MESH_MAX_VERTS, "%s: %d / %d vertices outside 1..%d", what, Va, Vb,
                DIR_MESH_MAX_VERTS);
    DIR_REQUIRE(Fa > 0 && Fb > 0 && Fa <= DIR_MESH_MAX_FACES && Fb <= DIR_MESH_MAX_FACES, "%s: %d / %d faces outside 1..%d", what, Fa, Fb,
                DIR_MESH_MAX_FACES);
    return DIR_OK;
}

}  // namespace

extern "C" int dir_mesh_penetration(const float* verts_a, const int32_t* faces_a, const float* verts_b, const int32_t* faces_b, int B, int Va,
                                    int Fa, int Vb, int Fb, float* winding, float* dist, int32_t* count, float* max_depth, float* sum_depth,
                                    void* stream) {
    if (int rc = check_meshes("dir_mesh_penetration", verts_a, faces_a, verts_b, faces_b, B, Va, Fa, Vb, Fb)) return rc;
    DIR_REQUIRE(count && max_depth && sum_depth, "dir_mesh_penetration: null pointer (count / max_depth / sum_depth)");
    // as few passes over the query vertices as 1024 threads allow, in whole waves (MANO: 778 vertices on 832 threads); a function of the
    // mesh sizes alone, so a sample's sums are the same in any batch
    const int vq = Va > Vb ? Va : Vb, passes = (vq + 1023) / 1024, T = ((vq + passes - 1) / passes + 63) / 64 * 64;
    DIR_LAUNCH(penetration_kernel, dim3(2 * B), dim3(T), 0, (hipStream_t)stream, verts_a, faces_a, verts_b, faces_b, Va, Fa, Vb, Fb, winding,
               dist, count, max_depth, sum_depth);
    return dir::check_launch("dir_mesh_penetration");
}

extern "C" int dir_mesh_intersection_volume(const float* verts_a, const int32_t* faces_a, const float* verts_b, const int32_t* faces_b, int B,
                                            int Va, int Fa, int Vb, int Fb, float h, int max_cells, float* volume, int32_t* n_both,
                                            int32_t* cells, void* stream) {
    if (int rc = check_meshes("dir_mesh_intersection_volume", verts_a, faces_a, verts_b, faces_b, B, Va, Fa, Vb, Fb)) return rc;
    DIR_REQUIRE(volume && n_both && cells, "dir_mesh_intersection_volume: null pointer (volume / n_both / cells)");
    DIR_REQUIRE(h > 0.f && h < INFINITY, "dir_mesh_intersection_volume: pitch h = %g must be positive and finite", (double)h);
    DIR_REQUIRE(max_cells > 0 && max_cells <= DIR_MESH_MAX_CELLS, "dir_mesh_intersection_volume: max_cells %d outside 1..%d", max_cells,
                DIR_MESH_MAX_CELLS);
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(n_both, 0, (size_t)B * sizeof(int32_t), s) != hipSuccess) return dir::check_launch("dir_mesh_intersection_volume (clear)");
    DIR_LAUNCH(volume_kernel, dim3(B * VG), dim3(VT), 0, s, verts_a, faces_a, verts_b, faces_b, Va, Fa, Vb, Fb, h, max_cells, n_both, cells);
    if (int rc = dir::check_launch("dir_mesh_intersection_volume")) return rc;
    DIR_LAUNCH(volume_finish_kernel, dim3((B + 255) / 256), dim3(256), 0, s, n_both, cells, h, max_cells, B, volume);
    return dir::check_launch("dir_mesh_intersection_volume (finish)");
}
