// Two-hand mesh rasteriser: dataset/prepare_data.py:174-214 (render_data) through utils/vis_utils.py:110-136, 253-356
// (mano_two_hands_renderer: MeshRasterizer + HardPhongShader + AmbientLights) for a batch on the GPU.
//
//   bin_kernel     one thread per (image, face): the face's screen box as a range of 16x16 tiles, packed in one word
//   raster_kernel  one workgroup per (image, 16x16 tile): the faces whose box touches the tile are compacted into LDS in face-index
//                  order (ballot + prefix sum), each lane scans that list for its pixel with the exact rules below, and the pixel is
//                  shaded and written once.  No atomics; the result does not depend on the schedule.
//
// The rules restate pytorch3d >= 0.7's rasterize_meshes with the reference's settings (blur_radius 0, faces_per_pixel 1,
// perspective-correct barycentrics, no culling, no z clipping), float32 operation by operation, no fused multiply-add:
//   camera       fx = -K00*2/S, fy = -K11*2/S, px = -K02*2/S + 1, py = -K12*2/S + 1 (vis_utils.py:149-156);
//                x_ndc = (fx*X + px*Z) / Z, y_ndc = (fy*Y + py*Z) / Z, depth = Z; no clamp on the division
//   pixel        output row r, column c samples x = 1 - (2c+1)/S, y = 1 - (2r+1)/S (pixel (c + 0.5, r + 0.5) in OpenCV terms)
//   edge         E(p,a,b) = (p.x-a.x)*(b.y-a.y) - (p.y-a.y)*(b.x-a.x)
//   zero area    a face with |E(v0,v1,v2)| <= 1e-8 is skipped
//   barycentric  area = E(v2,v0,v1) + 1e-8; w0 = E(p,v1,v2)/area, w1 = E(p,v2,v0)/area, w2 = E(p,v0,v1)/area
//   perspective  t0 = w0*z1*z2, t1 = z0*w1*z2, t2 = z0*z1*w2, d = max(t0+t1+t2, 1e-8) (a NaN sum gives 1e-8), b_i = t_i/d
//   depth        pz = b0*z0 + b1*z1 + b2*z2; the face is skipped at the pixel when pz < 0
//   coverage     b0 > 0 && b1 > 0 && b2 > 0, strictly (NaN does not cover)
//   depth test   the first covering face is taken; a later one replaces it only when its pz is strictly smaller, so on a tie the
//                lower face index wins
//   shading      texel t = b0*c0 + b1*c1 + b2*c2 per channel, left to right (HardPhongShader with AmbientLights and the default
//                Materials / BlendParams: ambient 1, no diffuse or specular term); background 1.0
//   frames       what cv.imwrite receives (prepare_data.py:206-214): u8 = round_half_even(fl32(fl32(t/255) * 255)) saturated to
//                [0, 255], so the background is 1; colour image (render_densepose / render_mask): fl32(t/255), background fl32(1/255)
//   mask         left vertices (0, 0, 255), right vertices (0, 255, 0), in array channel order (vis_utils.py:332-336)
//
// The tile filter is conservative: a face is listed for every tile its screen box, grown by one pixel and by 2^-10 of the box's
// size, touches; a face with a vertex at Z <= 0 or a non-finite projected coordinate is listed everywhere (with vertices behind the
// camera the rules above can cover pixels outside the box).  Inside the grown box the exact rules decide, so the output equals a
// loop over all faces.  A float edge test can flip sign only within ~1e-6 of the box's size from an edge's line, which the growth
// covers for every face whose sharpest angle exceeds ~1e-4 rad.  A face index outside 0..1555 is never read: the face is skipped
// (the Python layer rejects such tables where they are loaded).
#include "dir_common.h"

namespace {

constexpr int NV = DIR_RENDER_VERTS, NF = DIR_RENDER_FACES, NV_HAND = NV / 2;
constexpr int TILE = 16, TPX = TILE * TILE;
constexpr unsigned EMPTY = 0x000000FFu;            // tile range (c0 = 255, c1 = 0, ...): touches no tile
constexpr unsigned EVERYWHERE = 0xFF00FF00u;       // (c0 = 0, c1 = 255, r0 = 0, r1 = 255): touches every tile

struct Cam { float fx, fy, px, py; };

__device__ __forceinline__ Cam camera(const float* K, int S) {
#pragma clang fp contract(off)
    const float s = (float)S;
    Cam c;
    c.fx = -K[0] * 2.f / s;
    c.fy = -K[4] * 2.f / s;
    c.px = -K[2] * 2.f / s + 1.f;
    c.py = -K[5] * 2.f / s + 1.f;
    return c;
}

__device__ __forceinline__ void project(const Cam& c, const float* v, float& x, float& y, float& z) {
#pragma clang fp contract(off)
    const float X = v[0], Y = v[1], Z = v[2];
    x = (c.fx * X + c.px * Z) / Z;
    y = (c.fy * Y + c.py * Z) / Z;
    z = Z;
}

__device__ __forceinline__ float edge(float px, float py, float ax, float ay, float bx, float by) {
#pragma clang fp contract(off)
    return (px - ax) * (by - ay) - (py - ay) * (bx - ax);
}

__device__ __forceinline__ bool face_ok(const int* f) {
    return (unsigned)f[0] < (unsigned)NV && (unsigned)f[1] < (unsigned)NV && (unsigned)f[2] < (unsigned)NV;
}

// screen range [lo, hi] (NDC, grown) -> the pixel index range it can touch, given that index i samples 1 - (2i+1)/S; false if empty
__device__ __forceinline__ bool pixel_range(float lo, float hi, int S, int& i0, int& i1) {
    const float s = (float)S;
    float a = floorf(((1.f - hi) * s - 1.f) * 0.5f), b = ceilf(((1.f - lo) * s - 1.f) * 0.5f);
    a = fmaxf(a, 0.f);
    b = fminf(b, s - 1.f);
    if (!(a <= b)) return false;
    i0 = (int)a;
    i1 = (int)b;
    return true;
}

__global__ __launch_bounds__(256) void bin_kernel(const float* __restrict__ verts, const int* __restrict__ faces, const float* __restrict__ K,
                                                  unsigned* __restrict__ ranges, int B, int S) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= B * NF) return;
    const int b = i / NF, f = i - b * NF;
    const int* fi = faces + f * 3;
    if (!face_ok(fi)) { ranges[i] = EMPTY; return; }
    const Cam cam = camera(K + b * 9, S);
    const float* V = verts + (long long)b * NV * 3;
    float x[3], y[3], z[3];
    for (int k = 0; k < 3; ++k) project(cam, V + fi[k] * 3, x[k], y[k], z[k]);
    if (fabsf(edge(x[0], y[0], x[1], y[1], x[2], y[2])) <= 1e-8f) { ranges[i] = EMPTY; return; }
    bool finite = true, front = true;
    for (int k = 0; k < 3; ++k) {
        finite = finite && isfinite(x[k]) && isfinite(y[k]);
        front = front && z[k] > 0.f;
    }
    if (!finite || !front) { ranges[i] = EVERYWHERE; return; }
    const float xl = fminf(fminf(x[0], x[1]), x[2]), xh = fmaxf(fmaxf(x[0], x[1]), x[2]);
    const float yl = fminf(fminf(y[0], y[1]), y[2]), yh = fmaxf(fmaxf(y[0], y[1]), y[2]);
    const float grow = 2.f / (float)S + fmaxf(xh - xl, yh - yl) * 0x1p-10f;
    int c0, c1, r0, r1;
    if (!pixel_range(xl - grow, xh + grow, S, c0, c1) || !pixel_range(yl - grow, yh + grow, S, r0, r1)) { ranges[i] = EMPTY; return; }
    ranges[i] = (unsigned)(c0 / TILE) | ((unsigned)(c1 / TILE) << 8) | ((unsigned)(r0 / TILE) << 16) | ((unsigned)(r1 / TILE) << 24);
}

struct RasterArgs {
    const float* verts;
    const int* faces;
    const float* K;
    const float* colors;
    const unsigned* ranges;
    int* pix_to_face;
    float *zbuf, *bary, *color_f32;
    unsigned char *mask, *color_u8;
    int B, S;
};

__device__ __forceinline__ unsigned char frame_u8(float t) {
#pragma clang fp contract(off)
    const float v = rintf((t / 255.f) * 255.f);                            // saturate_cast<uchar>(float): round half to even, clamp
    return (unsigned char)(v > 0.f ? (v < 255.f ? v : 255.f) : 0.f);     // NaN -> 0
}

__global__ __launch_bounds__(TPX) void raster_kernel(RasterArgs a) {
#pragma clang fp contract(off)
    __shared__ float fv[TPX * 9];
    __shared__ int fid[TPX];
    __shared__ int wcount[TPX / 64];
    const int S = a.S, tiles = (S + TILE - 1) / TILE, b = blockIdx.y;
    const int tr = blockIdx.x / tiles, tc = blockIdx.x - tr * tiles;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int r = tr * TILE + (tid >> 4), c = tc * TILE + (tid & 15);
    const float s = (float)S;
    const float px = 1.f - (float)(2 * c + 1) / s, py = 1.f - (float)(2 * r + 1) / s;
    const Cam cam = camera(a.K + b * 9, S);
    const float* V = a.verts + (long long)b * NV * 3;
    const unsigned* rg = a.ranges + (long long)b * NF;
    int best = -1;
    float bz = 0.f, bb0 = 0.f, bb1 = 0.f, bb2 = 0.f;
    for (int base = 0; base < NF; base += TPX) {
        const int f = base + tid;
        bool hit = false;
        if (f < NF) {
            const unsigned w = rg[f];
            const int c0 = w & 255, c1 = (w >> 8) & 255, r0 = (w >> 16) & 255, r1 = w >> 24;
            hit = c0 <= tc && tc <= c1 && r0 <= tr && tr <= r1;
        }
        const unsigned long long m = __ballot(hit);
        if (lane == 0) wcount[wave] = __popcll(m);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < TPX / 64; ++w) {
            before += w < wave ? wcount[w] : 0;
            total += wcount[w];
        }
        if (hit) {
            const int slot = before + __popcll(m & ((1ull << lane) - 1ull));
            const int* fi = a.faces + f * 3;
            fid[slot] = f;
            for (int k = 0; k < 3; ++k) project(cam, V + fi[k] * 3, fv[slot * 9 + 3 * k], fv[slot * 9 + 3 * k + 1], fv[slot * 9 + 3 * k + 2]);
        }
        __syncthreads();
        for (int j = 0; j < total; ++j) {
            const float* q = fv + j * 9;
            const float x0 = q[0], y0 = q[1], z0 = q[2], x1 = q[3], y1 = q[4], z1 = q[5], x2 = q[6], y2 = q[7], z2 = q[8];
            // listed faces passed the zero-area rule in bin_kernel (same projection, same operations)
            const float area = edge(x2, y2, x0, y0, x1, y1) + 1e-8f;
            const float e0 = edge(px, py, x1, y1, x2, y2), e1 = edge(px, py, x2, y2, x0, y0), e2 = edge(px, py, x0, y0, x1, y1);
            // with every z > 0, b_i > 0 needs t_i > 0, i.e. w_i = e_i / area > 0: e_i and area of one strict sign.  Skipping the
            // divisions when that fails changes no result; faces with a vertex at z <= 0 (or NaN) take the full path.
            if (z0 > 0.f && z1 > 0.f && z2 > 0.f &&
                !(area > 0.f ? (e0 > 0.f && e1 > 0.f && e2 > 0.f) : (area < 0.f && e0 < 0.f && e1 < 0.f && e2 < 0.f)))
                continue;
            const float w0 = e0 / area, w1 = e1 / area, w2 = e2 / area;
            const float t0 = w0 * z1 * z2, t1 = z0 * w1 * z2, t2 = z0 * z1 * w2;
            const float sum = t0 + t1 + t2;
            const float d = sum > 1e-8f ? sum : 1e-8f;
            const float b0 = t0 / d, b1 = t1 / d, b2 = t2 / d;
            if (!(b0 > 0.f && b1 > 0.f && b2 > 0.f)) continue;
            const float pz = b0 * z0 + b1 * z1 + b2 * z2;
            if (pz < 0.f) continue;
            if (best < 0 || pz < bz) {
                best = fid[j];
                bz = pz; bb0 = b0; bb1 = b1; bb2 = b2;
            }
        }
        __syncthreads();                                                   // the list is rewritten by the next chunk
    }
    if (r >= S || c >= S) return;
    const long long p = ((long long)b * S + r) * S + c;
    if (a.pix_to_face) a.pix_to_face[p] = best;
    if (a.zbuf) a.zbuf[p] = best < 0 ? -1.f : bz;
    if (a.bary) {
        a.bary[p * 3 + 0] = best < 0 ? -1.f : bb0;
        a.bary[p * 3 + 1] = best < 0 ? -1.f : bb1;
        a.bary[p * 3 + 2] = best < 0 ? -1.f : bb2;
    }
    int vi[3] = {0, 0, 0};
    if (best >= 0) {
        const int* fi = a.faces + best * 3;
        vi[0] = fi[0]; vi[1] = fi[1]; vi[2] = fi[2];
    }
    if (a.mask) {
        float t[3] = {0.f, 0.f, 0.f};
        for (int ch = 0; ch < 3; ++ch) {
            float cv[3];
            for (int k = 0; k < 3; ++k) cv[k] = ch == (vi[k] < NV_HAND ? 2 : 1) ? 255.f : 0.f;
            t[ch] = best < 0 ? 1.f : bb0 * cv[0] + bb1 * cv[1] + bb2 * cv[2];
        }
        for (int ch = 0; ch < 3; ++ch) a.mask[p * 3 + ch] = frame_u8(t[ch]);
    }
    if (a.color_u8 || a.color_f32) {
        for (int ch = 0; ch < 3; ++ch) {
            const float t = best < 0 ? 1.f : bb0 * a.colors[vi[0] * 3 + ch] + bb1 * a.colors[vi[1] * 3 + ch] + bb2 * a.colors[vi[2] * 3 + ch];
            if (a.color_u8) a.color_u8[p * 3 + ch] = frame_u8(t);
            if (a.color_f32) a.color_f32[p * 3 + ch] = t / 255.f;
        }
    }
}

}  // namespace

extern "C" long long dir_render_workspace_bytes(int B) {
    return B > 0 ? (long long)B * NF * (long long)sizeof(unsigned) : 0;
}

extern "C" int dir_render_two_hands(const float* verts, const int32_t* faces, const float* K, const float* colors, int B, int S,
                                    void* workspace, long long workspace_bytes, int32_t* pix_to_face, float* zbuf, float* bary,
                                    uint8_t* mask, uint8_t* color_u8, float* color_f32, void* stream) {
    if (B == 0) return DIR_OK;
    DIR_REQUIRE(verts && faces && K && workspace && B > 0 && B <= DIR_RENDER_MAX_BATCH,
                "dir_render_two_hands: bad args (null pointer or B %d outside 1..%d)", B, DIR_RENDER_MAX_BATCH);
    DIR_REQUIRE(S >= DIR_RENDER_MIN_SIZE && S <= DIR_RENDER_MAX_SIZE, "dir_render_two_hands: S %d outside %d..%d", S, DIR_RENDER_MIN_SIZE,
                DIR_RENDER_MAX_SIZE);
    DIR_REQUIRE(workspace_bytes >= dir_render_workspace_bytes(B), "dir_render_two_hands: workspace of %lld bytes, %lld needed",
                workspace_bytes, dir_render_workspace_bytes(B));
    DIR_REQUIRE(colors || (!color_u8 && !color_f32), "dir_render_two_hands: a colour output needs the colour table");
    DIR_REQUIRE(pix_to_face || zbuf || bary || mask || color_u8 || color_f32, "dir_render_two_hands: no output requested");
    hipStream_t s = (hipStream_t)stream;
    unsigned* ranges = (unsigned*)workspace;
    const int n = B * NF;
    DIR_LAUNCH(bin_kernel, dim3((n + 255) / 256), dim3(256), 0, s, verts, faces, K, ranges, B, S);
    if (int rc = dir::check_launch("dir_render_two_hands (bin)")) return rc;
    RasterArgs a;
    a.verts = verts; a.faces = faces; a.K = K; a.colors = colors; a.ranges = ranges;
    a.pix_to_face = pix_to_face; a.zbuf = zbuf; a.bary = bary; a.color_f32 = color_f32; a.mask = mask; a.color_u8 = color_u8;
    a.B = B; a.S = S;
    const int tiles = (S + TILE - 1) / TILE;
    DIR_LAUNCH(raster_kernel, dim3(tiles * tiles, B), dim3(TPX), 0, s, a);
    return dir::check_launch("dir_render_two_hands");
}
