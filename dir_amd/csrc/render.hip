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
//
// Shaded and orthographic rendering (dir_render_shaded: render_rgb / render_rgb_orth and the scale= / trans2d= cameras of
// vis_utils.py:138-149, 278-330) is the same raster kernel in two more instantiations, with these further rules.  Only + - * /, sqrt,
// and compares are used, float32 operation by operation; max(x, m) below means x > m ? x : m (a NaN gives m):
//   normals      pytorch3d's verts_normals_packed in world space: for every face, corner 0 adds cross(v1-v0, v2-v0) to its vertex,
//                corner 1 cross(v2-v1, v0-v1), corner 2 cross(v0-v2, v1-v2), with cross(u, w) = (u.y*w.z - u.z*w.y, u.z*w.x - u.x*w.z,
//                u.x*w.y - u.y*w.x); then n / max(sqrt(n.x*n.x + n.y*n.y + n.z*n.z), 1e-6).  pytorch3d scatters with atomics; here
//                each vertex gathers its (face, corner) pairs in ascending face index, then corner, from an adjacency that
//                adjacency_kernel builds once per face table.  Faces with an index outside 0..1555 add nothing.
//   orthographic R = diag(-1,-1,1), T = (0,0,10), focal 2*scale, principal point -trans2d (vis_utils.py:138-149):
//                x_ndc = (2*scale)*(-X) + (-trans2d.x), y likewise, depth = Z + 10; camera centre (0,0,-10) (perspective: (0,0,0)).
//                No perspective correction: b_i = w_i, pz = w0*z0 + w1*z1 + w2*z2.  Every other raster rule is as above.  The tile
//                filter uses the projected box as it is: b_i > 0 holds only inside the screen triangle whatever the depths are
//                (a non-finite coordinate lists the face everywhere).
//   shading      HardPhongShader with PointLights, per covered pixel, sums left to right, b_i the barycentrics that are output:
//                p = b0*v0 + b1*v1 + b2*v2 (world), m = b0*n0 + b1*n1 + b2*n2, n = m / max(|m|, 1e-6);
//                l = location - p, d = l / max(|l|, 1e-6), c = n.d; diffuse = diffuse_colour * max(c, 0);
//                v = centre - p, view = v / max(|v|, 1e-6), r = -d + 2*(c*n), a = c > 0 ? max(view.r, 0) : 0,
//                specular = specular_colour * a^64 (six successive squarings: torch.pow differs by rounding only);
//                colour = (ambient + diffuse) * texel + specular; background 1.0; image = fl32(colour / 255).
//                With ambient 1 and no diffuse or specular colour this is the texel above, bit for bit.
//   overlay      frame_u8(colour) as above where a face covers the pixel, the background frame's bytes elsewhere (1 without a frame)
//   joints       dir_render_joints draws predicted 2-D joints over a uint8 picture by a rule of this project's own (NOT OpenCV's
//                drawing, whose anti-aliasing is not pinned anywhere): a joint uv in -1..1 sits at P = (uv + 1) * S / 2 where pixel
//                (c, r) has its centre at (c + 0.5, r + 0.5); a primitive covers a pixel by cov = clamp(rad + 0.5 - dist, 0, 1), dist
//                the distance from the pixel centre to the joint (disc) or to the bone's segment (t = clamp((p-a).(b-a) / |b-a|^2,
//                0, 1), 0 for a zero-length bone; q = a + t*(b-a)); o = o + cov * (colour - o) per channel in float32, in the fixed
//                order left hand then right hand, each its 20 bones then its 21 joints; the byte is frame_u8's rounding of o.
//                Joint k > 0 belongs to finger (k-1)/4, bone j joins joint (j%4 ? j : 0) to joint j+1 and takes finger j/4's colour.
// pytorch3d composes its camera transforms as 4x4 matrix products, so against pytorch3d itself these would agree to rounding only.
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

// orthographic: Cam holds fx = fy = 2*scale, px = -trans2d.x, py = -trans2d.y
__device__ __forceinline__ Cam camera_ortho(const float* scale, const float* trans2d, int b) {
#pragma clang fp contract(off)
    Cam c;
    c.fx = c.fy = 2.f * scale[b];
    c.px = -trans2d[2 * b];
    c.py = -trans2d[2 * b + 1];
    return c;
}

__device__ __forceinline__ void project_ortho(const Cam& c, const float* v, float& x, float& y, float& z) {
#pragma clang fp contract(off)
    x = c.fx * (-v[0]) + c.px;
    y = c.fy * (-v[1]) + c.py;
    z = v[2] + 10.f;
}

template <bool ORTHO>
__device__ __forceinline__ Cam camera_of(const float* K, const float* scale, const float* trans2d, int b, int S) {
    if constexpr (ORTHO) return camera_ortho(scale, trans2d, b);
    else return camera(K + b * 9, S);
}

template <bool ORTHO>
__device__ __forceinline__ void project_of(const Cam& c, const float* v, float& x, float& y, float& z) {
    if constexpr (ORTHO) project_ortho(c, v, x, y, z);
    else project(c, v, x, y, z);
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

template <bool ORTHO>
__global__ __launch_bounds__(256) void bin_kernel(const float* __restrict__ verts, const int* __restrict__ faces, const float* __restrict__ K,
                                                  const float* __restrict__ scale, const float* __restrict__ trans2d,
                                                  unsigned* __restrict__ ranges, int B, int S) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= B * NF) return;
    const int b = i / NF, f = i - b * NF;
    const int* fi = faces + f * 3;
    if (!face_ok(fi)) { ranges[i] = EMPTY; return; }
    const Cam cam = camera_of<ORTHO>(K, scale, trans2d, b, S);
    const float* V = verts + (long long)b * NV * 3;
    float x[3], y[3], z[3];
    for (int k = 0; k < 3; ++k) project_of<ORTHO>(cam, V + fi[k] * 3, x[k], y[k], z[k]);
    if (fabsf(edge(x[0], y[0], x[1], y[1], x[2], y[2])) <= 1e-8f) { ranges[i] = EMPTY; return; }
    bool finite = true, front = true;
    for (int k = 0; k < 3; ++k) {
        finite = finite && isfinite(x[k]) && isfinite(y[k]);
        front = front && (ORTHO || z[k] > 0.f);                           // orthographic: coverage does not depend on the depths
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

// dir_render_shaded: the camera is K or (scale, trans2d); normals / lights / background feed the Phong epilogue
struct ShadeArgs {
    const float* verts;
    const int* faces;
    const float *K, *scale, *trans2d;
    const float* colors;
    const float* normals;
    const unsigned* ranges;
    const unsigned char* background;
    int* pix_to_face;
    float *zbuf, *bary, *shaded_f32;
    unsigned char* overlay_u8;
    float ambient[3], diffuse[3], specular[3], location[3];
    int B, S;
};

__device__ __forceinline__ void normalize3(float x, float y, float z, float eps, float& ox, float& oy, float& oz) {
#pragma clang fp contract(off)
    const float len = __builtin_sqrtf(x * x + y * y + z * z);
    const float den = len > eps ? len : eps;
    ox = x / den; oy = y / den; oz = z / den;
}

// MODE 0: dir_render_two_hands (perspective, ambient texel), A = RasterArgs.  MODE 1 / 2: dir_render_shaded under the perspective /
// orthographic camera, A = ShadeArgs.
template <int MODE, class A>
__global__ __launch_bounds__(TPX) void raster_kernel(A a) {
#pragma clang fp contract(off)
    constexpr bool ORTHO = MODE == 2;
    __shared__ float fv[TPX * 9];
    __shared__ int fid[TPX];
    __shared__ int wcount[TPX / 64];
    const int S = a.S, tiles = (S + TILE - 1) / TILE, b = blockIdx.y;
    const int tr = blockIdx.x / tiles, tc = blockIdx.x - tr * tiles;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int r = tr * TILE + (tid >> 4), c = tc * TILE + (tid & 15);
    const float s = (float)S;
    const float px = 1.f - (float)(2 * c + 1) / s, py = 1.f - (float)(2 * r + 1) / s;
    Cam cam;
    if constexpr (MODE == 0) cam = camera(a.K + b * 9, S);
    else cam = camera_of<ORTHO>(a.K, a.scale, a.trans2d, b, S);
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
            for (int k = 0; k < 3; ++k) project_of<ORTHO>(cam, V + fi[k] * 3, fv[slot * 9 + 3 * k], fv[slot * 9 + 3 * k + 1], fv[slot * 9 + 3 * k + 2]);
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
            float b0, b1, b2;
            if constexpr (ORTHO) {
                // b_i = e_i / area > 0 needs e_i and area of one strict sign, whatever the depths; a zero or NaN area takes the divisions
                if ((area > 0.f && !(e0 > 0.f && e1 > 0.f && e2 > 0.f)) || (area < 0.f && !(e0 < 0.f && e1 < 0.f && e2 < 0.f))) continue;
                b0 = e0 / area; b1 = e1 / area; b2 = e2 / area;
            } else {
                if (z0 > 0.f && z1 > 0.f && z2 > 0.f &&
                    !(area > 0.f ? (e0 > 0.f && e1 > 0.f && e2 > 0.f) : (area < 0.f && e0 < 0.f && e1 < 0.f && e2 < 0.f)))
                    continue;
                const float w0 = e0 / area, w1 = e1 / area, w2 = e2 / area;
                const float t0 = w0 * z1 * z2, t1 = z0 * w1 * z2, t2 = z0 * z1 * w2;
                const float sum = t0 + t1 + t2;
                const float d = sum > 1e-8f ? sum : 1e-8f;
                b0 = t0 / d; b1 = t1 / d; b2 = t2 / d;
            }
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
    if constexpr (MODE != 0) {
        if (!a.shaded_f32 && !a.overlay_u8) return;
        if (best < 0) {
            for (int ch = 0; ch < 3; ++ch) {
                if (a.shaded_f32) a.shaded_f32[p * 3 + ch] = 1.f / 255.f;
                if (a.overlay_u8) a.overlay_u8[p * 3 + ch] = a.background ? a.background[p * 3 + ch] : frame_u8(1.f);
            }
            return;
        }
        const float* N = a.normals + (long long)b * NV * 3;
        float pw[3], m[3];
        for (int k = 0; k < 3; ++k) {
            pw[k] = bb0 * V[vi[0] * 3 + k] + bb1 * V[vi[1] * 3 + k] + bb2 * V[vi[2] * 3 + k];
            m[k] = bb0 * N[vi[0] * 3 + k] + bb1 * N[vi[1] * 3 + k] + bb2 * N[vi[2] * 3 + k];
        }
        float n[3], d[3], view[3];
        normalize3(m[0], m[1], m[2], 1e-6f, n[0], n[1], n[2]);
        normalize3(a.location[0] - pw[0], a.location[1] - pw[1], a.location[2] - pw[2], 1e-6f, d[0], d[1], d[2]);
        const float cosa = n[0] * d[0] + n[1] * d[1] + n[2] * d[2];
        const float dif = cosa > 0.f ? cosa : 0.f;
        normalize3(0.f - pw[0], 0.f - pw[1], (ORTHO ? -10.f : 0.f) - pw[2], 1e-6f, view[0], view[1], view[2]);
        float r[3];
        for (int k = 0; k < 3; ++k) r[k] = -d[k] + 2.f * (cosa * n[k]);
        const float vr = view[0] * r[0] + view[1] * r[1] + view[2] * r[2];
        float al = cosa > 0.f ? (vr > 0.f ? vr : 0.f) : 0.f;
#pragma unroll
        for (int q = 0; q < 6; ++q) al = al * al;                              // a^64
        for (int ch = 0; ch < 3; ++ch) {
            const float t = bb0 * a.colors[vi[0] * 3 + ch] + bb1 * a.colors[vi[1] * 3 + ch] + bb2 * a.colors[vi[2] * 3 + ch];
            const float col = (a.ambient[ch] + a.diffuse[ch] * dif) * t + a.specular[ch] * al;
            if (a.shaded_f32) a.shaded_f32[p * 3 + ch] = col / 255.f;
            if (a.overlay_u8) a.overlay_u8[p * 3 + ch] = frame_u8(col);
        }
    } else {
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
}

// ---- vertex normals.  The adjacency: int32 offsets [NV + 1], then int32 entries [3 NF], entry = face * 4 + corner.
constexpr int ADJ_ENTRIES = 3 * NF, ADJ_INTS = NV + 1 + ADJ_ENTRIES;

// one workgroup; made once per face table.  Thread t owns vertices t and t + 1024: it counts, then lists, the (face, corner) pairs that
// name its vertex, walking the table in ascending face index, then corner
__global__ __launch_bounds__(1024) void adjacency_kernel(const int* __restrict__ faces, int* __restrict__ adj) {
    __shared__ int fl[NF * 3];
    __shared__ int start[NV + 1];
    const int tid = threadIdx.x;
    for (int f = tid; f < NF; f += 1024) {
        const int* fi = faces + f * 3;
        const bool ok = face_ok(fi);
        for (int k = 0; k < 3; ++k) fl[f * 3 + k] = ok ? fi[k] : -1;
    }
    __syncthreads();
    for (int v = tid; v < NV; v += 1024) {
        int n = 0;
        for (int e = 0; e < NF * 3; ++e) n += fl[e] == v;
        start[v + 1] = n;
    }
    __syncthreads();
    if (tid == 0) {
        start[0] = 0;
        for (int v = 0; v < NV; ++v) start[v + 1] += start[v];
    }
    __syncthreads();
    for (int v = tid; v <= NV; v += 1024) adj[v] = start[v];
    for (int v = tid; v < NV; v += 1024) {
        int o = start[v];
        for (int e = 0; e < NF * 3; ++e)
            if (fl[e] == v) adj[NV + 1 + o++] = (e / 3) * 4 + e % 3;
    }
}

// one thread per (image, vertex).  Offsets and entries are clamped and re-checked against the face table, so that an adjacency that was
// not made for this table can give wrong normals but never a read outside the tables.
__global__ __launch_bounds__(256) void normals_kernel(const float* __restrict__ verts, const int* __restrict__ faces, const int* __restrict__ adj,
                                                      float* __restrict__ normals, int B) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= B * NV) return;
    const int b = i / NV, v = i - b * NV;
    const float* V = verts + (long long)b * NV * 3;
    int o0 = adj[v], o1 = adj[v + 1];
    o0 = o0 < 0 ? 0 : (o0 > ADJ_ENTRIES ? ADJ_ENTRIES : o0);
    o1 = o1 < o0 ? o0 : (o1 > ADJ_ENTRIES ? ADJ_ENTRIES : o1);
    float nx = 0.f, ny = 0.f, nz = 0.f;
    for (int e = o0; e < o1; ++e) {
        const int w = adj[NV + 1 + e], f = w >> 2, k = w & 3;
        if ((unsigned)f >= (unsigned)NF || k > 2) continue;
        const int* fi = faces + f * 3;
        if (!face_ok(fi)) continue;
        const float* p = V + fi[k] * 3;
        const float* q = V + fi[k == 2 ? 0 : k + 1] * 3;
        const float* r = V + fi[k == 0 ? 2 : k - 1] * 3;
        const float ux = q[0] - p[0], uy = q[1] - p[1], uz = q[2] - p[2];
        const float wx = r[0] - p[0], wy = r[1] - p[1], wz = r[2] - p[2];
        nx = nx + (uy * wz - uz * wy);
        ny = ny + (uz * wx - ux * wz);
        nz = nz + (ux * wy - uy * wx);
    }
    float ox, oy, oz;
    normalize3(nx, ny, nz, 1e-6f, ox, oy, oz);
    normals[(long long)i * 3 + 0] = ox;
    normals[(long long)i * 3 + 1] = oy;
    normals[(long long)i * 3 + 2] = oz;
}

// ---- predicted 2-D joints over a picture (the rule is in the header comment)
__constant__ float JOINT_PALETTE[6][3] = {{255.f, 255.f, 255.f}, {60.f, 60.f, 230.f}, {60.f, 200.f, 230.f},
                                          {80.f, 220.f, 80.f},   {230.f, 180.f, 60.f}, {220.f, 80.f, 200.f}};      // wrist, thumb .. little finger

__device__ __forceinline__ float coverage(float rad, float dist) {
#pragma clang fp contract(off)
    const float x = rad + 0.5f - dist;
    return x > 0.f ? (x < 1.f ? x : 1.f) : 0.f;                               // NaN -> 0
}

__global__ __launch_bounds__(256) void joints_kernel(unsigned char* __restrict__ image, const float* __restrict__ uv_left,
                                                     const float* __restrict__ uv_right, int S, float joint_radius, float bone_radius) {
#pragma clang fp contract(off)
    __shared__ float P[2][21][2];
    const int b = blockIdx.y, tid = threadIdx.x;
    if (tid < 84) {
        const int h = tid / 42, k = tid - h * 42;
        const float uv = (h ? uv_right : uv_left)[b * 42 + k];
        P[h][k >> 1][k & 1] = (uv + 1.f) * (float)S / 2.f;
    }
    __syncthreads();
    const int i = blockIdx.x * 256 + tid;
    if (i >= S * S) return;
    const int r = i / S, c = i - r * S;
    const float px = (float)c + 0.5f, py = (float)r + 0.5f;
    unsigned char* pix = image + ((long long)b * S * S + i) * 3;
    float o[3] = {(float)pix[0], (float)pix[1], (float)pix[2]};
    bool touched = false;
    for (int h = 0; h < 2; ++h) {
        for (int j = 0; j < 20; ++j) {
            const float* A = P[h][j % 4 ? j : 0];
            const float* Bp = P[h][j + 1];
            const float abx = Bp[0] - A[0], aby = Bp[1] - A[1];
            const float l2 = abx * abx + aby * aby;
            float t = 0.f;
            if (l2 > 0.f) {
                t = ((px - A[0]) * abx + (py - A[1]) * aby) / l2;
                t = t > 0.f ? (t < 1.f ? t : 1.f) : 0.f;
            }
            const float dx = px - (A[0] + t * abx), dy = py - (A[1] + t * aby);
            const float cov = coverage(bone_radius, __builtin_sqrtf(dx * dx + dy * dy));
            if (cov > 0.f) {                                                  // cov = 0 leaves o as it is
                touched = true;
                for (int ch = 0; ch < 3; ++ch) o[ch] = o[ch] + cov * (JOINT_PALETTE[1 + j / 4][ch] - o[ch]);
            }
        }
        for (int k = 0; k < 21; ++k) {
            const float dx = px - P[h][k][0], dy = py - P[h][k][1];
            const float cov = coverage(joint_radius, __builtin_sqrtf(dx * dx + dy * dy));
            if (cov > 0.f) {
                touched = true;
                for (int ch = 0; ch < 3; ++ch) o[ch] = o[ch] + cov * (JOINT_PALETTE[k ? 1 + (k - 1) / 4 : 0][ch] - o[ch]);
            }
        }
    }
    if (!touched) return;
    for (int ch = 0; ch < 3; ++ch) {
        const float v = rintf(o[ch]);
        pix[ch] = (unsigned char)(v > 0.f ? (v < 255.f ? v : 255.f) : 0.f);
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
    DIR_LAUNCH(bin_kernel<false>, dim3((n + 255) / 256), dim3(256), 0, s, verts, faces, K, (const float*)nullptr, (const float*)nullptr, ranges, B, S);
    if (int rc = dir::check_launch("dir_render_two_hands (bin)")) return rc;
    RasterArgs a;
    a.verts = verts; a.faces = faces; a.K = K; a.colors = colors; a.ranges = ranges;
    a.pix_to_face = pix_to_face; a.zbuf = zbuf; a.bary = bary; a.color_f32 = color_f32; a.mask = mask; a.color_u8 = color_u8;
    a.B = B; a.S = S;
    const int tiles = (S + TILE - 1) / TILE;
    DIR_LAUNCH((raster_kernel<0, RasterArgs>), dim3(tiles * tiles, B), dim3(TPX), 0, s, a);
    return dir::check_launch("dir_render_two_hands");
}

extern "C" long long dir_render_adjacency_bytes(void) { return (long long)ADJ_INTS * (long long)sizeof(int); }

extern "C" int dir_render_adjacency(const int32_t* faces, void* adjacency, long long adjacency_bytes, void* stream) {
    DIR_REQUIRE(faces && adjacency, "dir_render_adjacency: null pointer");
    DIR_REQUIRE(adjacency_bytes >= dir_render_adjacency_bytes(), "dir_render_adjacency: buffer of %lld bytes, %lld needed", adjacency_bytes,
                dir_render_adjacency_bytes());
    DIR_LAUNCH(adjacency_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, faces, (int*)adjacency);
    return dir::check_launch("dir_render_adjacency");
}

extern "C" int dir_render_vertex_normals(const float* verts, const int32_t* faces, const void* adjacency, int B, float* normals, void* stream) {
    if (B == 0) return DIR_OK;
    DIR_REQUIRE(verts && faces && adjacency && normals && B > 0 && B <= DIR_RENDER_MAX_BATCH,
                "dir_render_vertex_normals: bad args (null pointer or B %d outside 1..%d)", B, DIR_RENDER_MAX_BATCH);
    const int n = B * NV;
    DIR_LAUNCH(normals_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, verts, faces, (const int*)adjacency, normals, B);
    return dir::check_launch("dir_render_vertex_normals");
}

extern "C" long long dir_render_shaded_workspace_bytes(int B) {
    return B > 0 ? (long long)B * (NF * (long long)sizeof(unsigned) + NV * 3 * (long long)sizeof(float)) : 0;
}

extern "C" int dir_render_shaded(const float* verts, const int32_t* faces, const void* adjacency, const float* K, const float* scale,
                                 const float* trans2d, const float* colors, const dir_render_lights* lights, const uint8_t* background, int B,
                                 int S, void* workspace, long long workspace_bytes, int32_t* pix_to_face, float* zbuf, float* bary,
                                 float* shaded_f32, uint8_t* overlay_u8, void* stream) {
    if (B == 0) return DIR_OK;
    DIR_REQUIRE(verts && faces && workspace && B > 0 && B <= DIR_RENDER_MAX_BATCH,
                "dir_render_shaded: bad args (null pointer or B %d outside 1..%d)", B, DIR_RENDER_MAX_BATCH);
    DIR_REQUIRE(S >= DIR_RENDER_MIN_SIZE && S <= DIR_RENDER_MAX_SIZE, "dir_render_shaded: S %d outside %d..%d", S, DIR_RENDER_MIN_SIZE,
                DIR_RENDER_MAX_SIZE);
    const bool ortho = scale || trans2d;
    DIR_REQUIRE((K != nullptr) != ortho, "dir_render_shaded: give exactly one camera, K or scale + trans2d (%s)", K ? "both given" : "none given");
    DIR_REQUIRE(!ortho || (scale && trans2d), "dir_render_shaded: the orthographic camera needs both scale and trans2d");
    DIR_REQUIRE(workspace_bytes >= dir_render_shaded_workspace_bytes(B), "dir_render_shaded: workspace of %lld bytes, %lld needed",
                workspace_bytes, dir_render_shaded_workspace_bytes(B));
    const bool shade = shaded_f32 || overlay_u8;
    DIR_REQUIRE(!shade || (colors && lights && adjacency), "dir_render_shaded: a colour output needs the colour table, the lights and the adjacency");
    DIR_REQUIRE(!shade || lights->shininess == 64.f, "dir_render_shaded: shininess %g: only 64 is built", shade ? (double)lights->shininess : 0.0);
    DIR_REQUIRE(!background || overlay_u8, "dir_render_shaded: a background frame is read by overlay_u8 only");
    DIR_REQUIRE(pix_to_face || zbuf || bary || shade, "dir_render_shaded: no output requested");
    hipStream_t s = (hipStream_t)stream;
    unsigned* ranges = (unsigned*)workspace;
    float* normals = (float*)(ranges + (long long)B * NF);
    if (shade) {
        const int nv = B * NV;
        DIR_LAUNCH(normals_kernel, dim3((nv + 255) / 256), dim3(256), 0, s, verts, faces, (const int*)adjacency, normals, B);
        if (int rc = dir::check_launch("dir_render_shaded (normals)")) return rc;
    }
    const int n = B * NF;
    if (ortho) DIR_LAUNCH(bin_kernel<true>, dim3((n + 255) / 256), dim3(256), 0, s, verts, faces, K, scale, trans2d, ranges, B, S);
    else DIR_LAUNCH(bin_kernel<false>, dim3((n + 255) / 256), dim3(256), 0, s, verts, faces, K, scale, trans2d, ranges, B, S);
    if (int rc = dir::check_launch("dir_render_shaded (bin)")) return rc;
    ShadeArgs a;
    a.verts = verts; a.faces = faces; a.K = K; a.scale = scale; a.trans2d = trans2d; a.colors = colors; a.normals = normals; a.ranges = ranges;
    a.background = background; a.pix_to_face = pix_to_face; a.zbuf = zbuf; a.bary = bary; a.shaded_f32 = shaded_f32; a.overlay_u8 = overlay_u8;
    for (int k = 0; k < 3; ++k) {
        a.ambient[k] = shade ? lights->ambient[k] : 0.f;
        a.diffuse[k] = shade ? lights->diffuse[k] : 0.f;
        a.specular[k] = shade ? lights->specular[k] : 0.f;
        a.location[k] = shade ? lights->location[k] : 0.f;
    }
    a.B = B; a.S = S;
    const int tiles = (S + TILE - 1) / TILE;
    if (ortho) DIR_LAUNCH((raster_kernel<2, ShadeArgs>), dim3(tiles * tiles, B), dim3(TPX), 0, s, a);
    else DIR_LAUNCH((raster_kernel<1, ShadeArgs>), dim3(tiles * tiles, B), dim3(TPX), 0, s, a);
    return dir::check_launch("dir_render_shaded");
}

extern "C" int dir_render_joints(uint8_t* image, const float* uv_left, const float* uv_right, int B, int S, float joint_radius,
                                 float bone_radius, void* stream) {
    if (B == 0) return DIR_OK;
    DIR_REQUIRE(image && uv_left && uv_right && B > 0 && B <= DIR_RENDER_MAX_BATCH,
                "dir_render_joints: bad args (null pointer or B %d outside 1..%d)", B, DIR_RENDER_MAX_BATCH);
    DIR_REQUIRE(S >= DIR_RENDER_MIN_SIZE && S <= DIR_RENDER_MAX_SIZE, "dir_render_joints: S %d outside %d..%d", S, DIR_RENDER_MIN_SIZE,
                DIR_RENDER_MAX_SIZE);
    DIR_REQUIRE(joint_radius >= 0.f && joint_radius <= 64.f && bone_radius >= 0.f && bone_radius <= 64.f,
                "dir_render_joints: radii %g / %g outside 0..64", (double)joint_radius, (double)bone_radius);
    DIR_LAUNCH(joints_kernel, dim3((S * S + 255) / 256, B), dim3(256), 0, (hipStream_t)stream, image, uv_left, uv_right, S, joint_radius,
               bone_radius);
    return dir::check_launch("dir_render_joints");
}
