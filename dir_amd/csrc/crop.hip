// Hand crops from full frames: dataset/dataset_utils.py:26-58 (cut_img) as the reference's prepare_data.py:153-154 calls it, for frames of
// any size, plus the way a video is followed without a box per frame.  The rules are written out in include/dir_hip.h and restated in
// float64 numpy by tests/helpers/crop_ref.py (matrices) and tests/helpers/augment_ref.py::warp_affine_u8 (pixels).
//
//   box_kernel     a tight box per image -> the crop matrix (one lane per image)
//   mesh_kernel    one stage of the network's output + the matrix of its crop -> the next frame's matrix (one workgroup per image: the
//                  1 556 projected vertices go back to frame pixels in double, min / max through LDS)
//   crop_kernel    cv.warpAffine(INTER_LINEAR, BORDER_CONSTANT 0) of a ragged batch of frames; one lane makes four neighbouring output
//                  pixels and stores them as three dwords (12 B per lane, adjacent lanes on adjacent addresses)
#include "dir_common.h"
#include "warp_fixed.h"

namespace {

using namespace warp;

constexpr int NV = 778;
constexpr int PIX = 4;                                    // output pixels per lane of crop_kernel

// cut_img's matrix from the per-axis extremes; returns 1 and writes M, or returns 0 (M untouched)
__device__ __forceinline__ int crop_rule(double mnx, double mny, double mxx, double mxy, double ratio, double half, double* M) {
#pragma clang fp contract(off)
    if (!(isfinite(mnx) && isfinite(mny) && isfinite(mxx) && isfinite(mxy))) return 0;
    const double midx = (mnx + mxx) / 2., midy = (mny + mxy) / 2.;
    const double ex = mxx - mnx, ey = mxy - mny;
    const double L = (ex > ey ? ex : ey) / 2. / ratio;
    if (!(isfinite(L) && L > 0.)) return 0;
    const double s = half / L;
    if (!(s >= DIR_CROP_MIN_SCALE && s <= DIR_CROP_MAX_SCALE)) return 0;
    if (!(fabs(midx - L) <= DIR_CROP_MAX_COORD && fabs(midx + L) <= DIR_CROP_MAX_COORD && fabs(midy - L) <= DIR_CROP_MAX_COORD &&
          fabs(midy + L) <= DIR_CROP_MAX_COORD))
        return 0;
    M[0] = s; M[1] = 0.; M[2] = s * (L - midx);
    M[3] = 0.; M[4] = s; M[5] = s * (L - midy);
    return 1;
}

__global__ __launch_bounds__(64) void box_kernel(const float* __restrict__ boxes, int B, double ratio, double half, double* __restrict__ M,
                                                 int* __restrict__ valid) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const double x0 = boxes[b * 4 + 0], y0 = boxes[b * 4 + 1], x1 = boxes[b * 4 + 2], y1 = boxes[b * 4 + 3];
    double m[6] = {0., 0., 0., 0., 0., 0.};
    // NaN compares false both ways: it stays in one of the two extremes and crop_rule sees it
    const int ok = crop_rule(x0 < x1 ? x0 : x1, y0 < y1 ? y0 : y1, x0 < x1 ? x1 : x0, y0 < y1 ? y1 : y0, ratio, half, m);
#pragma unroll
    for (int i = 0; i < 6; ++i) M[b * 6 + i] = m[i];
    valid[b] = ok;
}

struct MeshArgs {
    const float *mesh[2], *proj[2];
    const double* M_prev;
    double* M_next;
    int* valid;
    double ratio, half, size;
};

__global__ __launch_bounds__(256) void mesh_kernel(MeshArgs a) {
#pragma clang fp contract(off)
    __shared__ double red[4][256];
    __shared__ int bad_s[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    double mp[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) mp[i] = a.M_prev[(long long)b * 6 + i];
    double mnx = INFINITY, mny = INFINITY, mxx = -INFINITY, mxy = -INFINITY;
    int bad = 0;
    for (int i = tid; i < 2 * NV; i += 256) {
        const int h = i >= NV, k = h ? i - NV : i;
        const float* v = a.mesh[h] + ((long long)b * NV + k) * 3;
        const float* p = a.proj[h] + (long long)b * 3;
        const float u = p[0] * v[0] + p[1], w = p[0] * v[1] + p[2];                    // float32: multiply, then add
        const double px = (((double)u + 1.) * a.size / 2. - mp[2]) / mp[0];
        const double py = (((double)w + 1.) * a.size / 2. - mp[5]) / mp[0];
        bad |= !(isfinite(px) && isfinite(py));
        mnx = px < mnx ? px : mnx; mxx = px > mxx ? px : mxx;
        mny = py < mny ? py : mny; mxy = py > mxy ? py : mxy;
    }
    red[0][tid] = mnx; red[1][tid] = mny; red[2][tid] = mxx; red[3][tid] = mxy;
    bad_s[tid] = bad;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) {
            red[0][tid] = red[0][tid + o] < red[0][tid] ? red[0][tid + o] : red[0][tid];
            red[1][tid] = red[1][tid + o] < red[1][tid] ? red[1][tid + o] : red[1][tid];
            red[2][tid] = red[2][tid + o] > red[2][tid] ? red[2][tid + o] : red[2][tid];
            red[3][tid] = red[3][tid + o] > red[3][tid] ? red[3][tid + o] : red[3][tid];
            bad_s[tid] |= bad_s[tid + o];
        }
        __syncthreads();
    }
    if (tid == 0) {
        double m[6];
        int ok = !bad_s[0] && crop_rule(red[0][0], red[1][0], red[2][0], red[3][0], a.ratio, a.half, m);
        if (!ok) {
#pragma unroll
            for (int i = 0; i < 6; ++i) m[i] = mp[i];                                  // the box holds
        }
#pragma unroll
        for (int i = 0; i < 6; ++i) a.M_next[(long long)b * 6 + i] = m[i];
        a.valid[b] = ok;
    }
}

struct CropArgs {
    const unsigned char* frames;
    long long bytes;
    const dir_frame_desc* descs;
    const double* M;
    const int* valid;
    unsigned char* out;
    int* status;
    int B, size;
};

struct Image {          // what one lane knows about the image its current pixel belongs to
    const unsigned char* f;
    long long stride;
    int h, w, status;
    double m[6];
};

__device__ __forceinline__ void load_image(const CropArgs& a, int b, Image& im) {
#pragma clang fp contract(off)
    const dir_frame_desc d = a.descs[b];
    im.f = a.frames; im.stride = 0; im.h = im.w = 0;
    if (a.valid && !a.valid[b]) { im.status = DIR_CROP_INVALID; return; }
    // every term is bounded before it is used, so nothing below overflows: offset <= bytes < 2^63, (h - 1) * stride < 2^36
    if (d.height < 1 || d.height > DIR_CROP_MAX_SIDE || d.width < 1 || d.width > DIR_CROP_MAX_SIDE || d.row_stride < 3ll * d.width ||
        d.row_stride > DIR_CROP_MAX_STRIDE || d.offset < 0 || d.offset > a.bytes ||
        (long long)(d.height - 1) * d.row_stride + 3ll * d.width > a.bytes - d.offset) {
        im.status = DIR_CROP_BAD_DESC;
        return;
    }
    invert_affine(a.M + (long long)b * 6, im.m);
    const double far = (double)(a.size - 1);
    const double rx = fabs(im.m[0]) * far + fabs(im.m[1]) * far + fabs(im.m[2]);
    const double ry = fabs(im.m[3]) * far + fabs(im.m[4]) * far + fabs(im.m[5]);
    if (!(rx <= DIR_CROP_MAX_COORD && ry <= DIR_CROP_MAX_COORD)) { im.status = DIR_CROP_BAD_MATRIX; return; }      // NaN / inf fail the comparison
    im.f = a.frames + d.offset; im.stride = d.row_stride; im.h = d.height; im.w = d.width; im.status = 0;
}

// one output pixel -> its three bytes, in bits 0..23
__device__ __forceinline__ unsigned crop_pixel(const Image& im, int x, int y) {
    if (im.status) return 0u;
    int sx, sy, fx, fy, w[4];
    warp_coord(im.m, x, y, sx, sy, fx, fy);
    warp_weights(fx, fy, w);
    int acc[3] = {0, 0, 0};
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int xx = sx + (t & 1), yy = sy + (t >> 1);
        if ((unsigned)xx < (unsigned)im.w && (unsigned)yy < (unsigned)im.h) {          // a tap outside the frame reads 0 and is never loaded
            const unsigned char* p = im.f + (long long)yy * im.stride + (long long)xx * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c] += (int)p[c] * w[t];
        }
    }
    return (unsigned)warp_round(acc[0]) | ((unsigned)warp_round(acc[1]) << 8) | ((unsigned)warp_round(acc[2]) << 16);
}

__global__ __launch_bounds__(256) void crop_kernel(CropArgs a) {
    const long long per = (long long)a.size * a.size, total = per * a.B;
    const long long g0 = (blockIdx.x * 256ll + threadIdx.x) * PIX;                     // the lane's first pixel, counted over the whole batch
    if (g0 >= total) return;
    // total <= 4096 * 1024 * 1024 = 2^32 and g0 < total, so the lane's one division is a 32-bit one; its other pixels follow by counting
    int b = (int)((unsigned)g0 / (unsigned)per);
    int p = (int)((unsigned)g0 - (unsigned)b * (unsigned)per);
    int y = p / a.size, x = p - y * a.size;
    Image im;
    int cur = -1;
    unsigned px[PIX];
#pragma unroll
    for (int j = 0; j < PIX; ++j) {
        px[j] = 0u;
        if (g0 + j >= total) continue;
        if (b != cur) {
            load_image(a, b, im);
            cur = b;
        }
        if (p == 0 && a.status) a.status[b] = im.status;
        px[j] = crop_pixel(im, x, y);
        ++p;
        if (++x == a.size) { x = 0; ++y; }
        if (p == (int)per) { p = 0; y = 0; ++b; }                                      // the next pixel opens the next image (x is 0 already)
    }
    unsigned char* o = a.out + g0 * 3;                                                 // 12 g0 / 4 bytes: dword aligned with `out`
    if (g0 + PIX <= total) {
        unsigned* o4 = reinterpret_cast<unsigned*>(o);
        o4[0] = px[0] | (px[1] << 24);
        o4[1] = (px[1] >> 8) | (px[2] << 16);
        o4[2] = (px[2] >> 16) | (px[3] << 8);
    } else {
        for (int j = 0; j < PIX && g0 + j < total; ++j) {
            o[j * 3 + 0] = (unsigned char)(px[j] & 255u);
            o[j * 3 + 1] = (unsigned char)((px[j] >> 8) & 255u);
            o[j * 3 + 2] = (unsigned char)((px[j] >> 16) & 255u);
        }
    }
}

bool crop_common_ok(int B, double ratio, int size) {
    return B > 0 && B <= DIR_CROP_MAX_BATCH && ratio > 0. && ratio <= 16. && size >= DIR_CROP_MIN_SIZE && size <= DIR_CROP_MAX_SIZE;
}

}  // namespace

extern "C" int dir_crop_matrices_from_boxes(const float* boxes, int B, double ratio, int size, double* M, int32_t* valid, void* stream) {
    if (B == 0) return DIR_OK;
    DIR_REQUIRE(boxes && M && valid, "dir_crop_matrices_from_boxes: null pointer");
    DIR_REQUIRE(crop_common_ok(B, ratio, size), "dir_crop_matrices_from_boxes: bad args (B %d outside 1..%d, ratio %g outside (0, 16] or size %d outside %d..%d)",
                B, DIR_CROP_MAX_BATCH, ratio, size, DIR_CROP_MIN_SIZE, DIR_CROP_MAX_SIZE);
    DIR_LAUNCH(box_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, boxes, B, ratio, (double)size / 2., M, valid);
    return dir::check_launch("dir_crop_matrices_from_boxes");
}

extern "C" int dir_crop_matrices_from_meshes(const float* mesh_left, const float* mesh_right, const float* proj_left, const float* proj_right,
                                             const double* M_prev, int B, double ratio, int size, double* M_next, int32_t* valid, void* stream) {
    if (B == 0) return DIR_OK;
    DIR_REQUIRE(mesh_left && mesh_right && proj_left && proj_right && M_prev && M_next && valid, "dir_crop_matrices_from_meshes: null pointer");
    DIR_REQUIRE(crop_common_ok(B, ratio, size), "dir_crop_matrices_from_meshes: bad args (B %d outside 1..%d, ratio %g outside (0, 16] or size %d outside %d..%d)",
                B, DIR_CROP_MAX_BATCH, ratio, size, DIR_CROP_MIN_SIZE, DIR_CROP_MAX_SIZE);
    MeshArgs a;
    a.mesh[0] = mesh_left; a.mesh[1] = mesh_right; a.proj[0] = proj_left; a.proj[1] = proj_right;
    a.M_prev = M_prev; a.M_next = M_next; a.valid = valid; a.ratio = ratio; a.half = (double)size / 2.; a.size = (double)size;
    DIR_LAUNCH(mesh_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, a);
    return dir::check_launch("dir_crop_matrices_from_meshes");
}

extern "C" int dir_crop_frames(const uint8_t* frames, long long frames_bytes, const dir_frame_desc* descs, const double* M, const int32_t* valid,
                               int B, int size, uint8_t* out, int32_t* status, void* stream) {
    if (B == 0) return DIR_OK;
    DIR_REQUIRE(frames && descs && M && out, "dir_crop_frames: null pointer");
    DIR_REQUIRE(crop_common_ok(B, 1., size) && frames_bytes > 0, "dir_crop_frames: bad args (B %d outside 1..%d, size %d outside %d..%d or %lld bytes of frames)",
                B, DIR_CROP_MAX_BATCH, size, DIR_CROP_MIN_SIZE, DIR_CROP_MAX_SIZE, frames_bytes);
    DIR_REQUIRE(((uintptr_t)out & 3) == 0, "dir_crop_frames: out must be 4-byte aligned");
    CropArgs a;
    a.frames = frames; a.bytes = frames_bytes; a.descs = descs; a.M = M; a.valid = valid; a.out = out; a.status = status; a.B = B; a.size = size;
    const long long lanes = ((long long)B * size * size + PIX - 1) / PIX;
    DIR_LAUNCH(crop_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    return dir::check_launch("dir_crop_frames");
}
