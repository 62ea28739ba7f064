// Hand crops from full frames: dataset/dataset_utils.py:26-58 (cut_img) as the reference's prepare_data.py:153-154 calls it, for frames of
// any size, plus the way a video is followed without a box per frame.  The rules are written out in include/dir_hip.h and restated in
// float64 numpy by tests/helpers/crop_ref.py (matrices) and tests/helpers/augment_ref.py::warp_affine_u8 (pixels).
//
//   box_kernel     a tight box per image -> the crop matrix (one lane per image)
//   mesh_kernel    one stage of the network's output + the matrix of its crop -> the next frame's matrix (one workgroup per image: the
//                  1 556 projected vertices go back to frame pixels in double, min / max through LDS)
//   crop_kernel    cv.warpAffine(INTER_LINEAR, BORDER_CONSTANT 0) of a ragged batch of frames; one lane makes four neighbouring output
//                  pixels and stores them as three dwords (12 B per lane, adjacent lanes on adjacent addresses)
//   area_kernel    the anti-aliased crop of the images whose matrix shrinks the frame (dir_crop_frames_area; the rule is Pillow's
//                  resize(BILINEAR, box), restated by tests/helpers/crop_area_ref.py): one workgroup per image x band of 16 output rows x
//                  tile of 32 output columns.  Its 22-bit coefficients are computed once, in double, into LDS (one lane per output
//                  position walking its taps); the source rows of the band are streamed through LDS in chunks of at most 8 rows (dword
//                  loads), filtered horizontally into a uint8 tile in LDS, and summed vertically into int registers
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
    int* area;          // dir_crop_frames_area only
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

// dir_crop_frames_area: does image b (loaded into im) get the anti-aliased rule?  A shrinking matrix below DIR_CROP_MIN_SCALE is refused here
__device__ __forceinline__ int area_rule(const CropArgs& a, int b, Image& im) {
    if (im.status) return 0;
    const double* M = a.M + (long long)b * 6;
    const double sx = M[0], sy = M[4];
    if (!(M[1] == 0. && M[3] == 0. && sx > 0. && sy > 0. && (sx < sy ? sx : sy) < 1.)) return 0;      // NaN fails: it went to BAD_MATRIX above
    if ((sx < sy ? sx : sy) < DIR_CROP_MIN_SCALE) { im.status = DIR_CROP_BAD_MATRIX; return 0; }
    return 1;
}

// AREA: the images that area_rule() takes are left to area_kernel -- their pixels are neither computed nor stored here
template <bool AREA> __global__ __launch_bounds__(256) void crop_kernel(CropArgs a) {
    const long long per = (long long)a.size * a.size, total = per * a.B;
    const long long g0 = (blockIdx.x * 256ll + threadIdx.x) * PIX;                     // the lane's first pixel, counted over the whole batch
    if (g0 >= total) return;
    // total <= 4096 * 1024 * 1024 = 2^32 and g0 < total, so the lane's one division is a 32-bit one; its other pixels follow by counting
    int b = (int)((unsigned)g0 / (unsigned)per);
    int p = (int)((unsigned)g0 - (unsigned)b * (unsigned)per);
    int y = p / a.size, x = p - y * a.size;
    Image im;
    int cur = -1, skip = 0;
    unsigned px[PIX], own = 0u;
#pragma unroll
    for (int j = 0; j < PIX; ++j) {
        px[j] = 0u;
        if (g0 + j >= total) continue;
        if (b != cur) {
            load_image(a, b, im);
            if constexpr (AREA) skip = area_rule(a, b, im);
            cur = b;
        }
        if (p == 0) {
            if (a.status) a.status[b] = im.status;
            if constexpr (AREA) {
                if (a.area) a.area[b] = skip;
            }
        }
        if (!skip) {
            px[j] = crop_pixel(im, x, y);
            own |= 1u << j;
        }
        ++p;
        if (++x == a.size) { x = 0; ++y; }
        if (p == (int)per) { p = 0; y = 0; ++b; }                                      // the next pixel opens the next image (x is 0 already)
    }
    unsigned char* o = a.out + g0 * 3;                                                 // 12 g0 / 4 bytes: dword aligned with `out`
    if (g0 + PIX <= total && (!AREA || own == (1u << PIX) - 1u)) {
        unsigned* o4 = reinterpret_cast<unsigned*>(o);
        o4[0] = px[0] | (px[1] << 24);
        o4[1] = (px[1] >> 8) | (px[2] << 16);
        o4[2] = (px[2] >> 16) | (px[3] << 8);
    } else {
        for (int j = 0; j < PIX && g0 + j < total; ++j) {
            if (AREA && !((own >> j) & 1u)) continue;
            o[j * 3 + 0] = (unsigned char)(px[j] & 255u);
            o[j * 3 + 1] = (unsigned char)((px[j] >> 8) & 255u);
            o[j * 3 + 2] = (unsigned char)((px[j] >> 16) & 255u);
        }
    }
}

// ---- the anti-aliased crop ----
constexpr int TX = 32, TY = 16;                          // output columns and rows per workgroup
constexpr int MAX_TAPS = 129;                            // 2 * 64 + 1: the window at DIR_CROP_MIN_SCALE; odd, so that the rows of Kx fall on different banks
constexpr int PREC = 22;                                 // Pillow's PRECISION_BITS
constexpr int ROWS = 8;                                  // source rows per chunk at most: 256 lanes = ROWS x TX horizontal sums
constexpr int SRC_BYTES = 16384;                         // the chunk of source rows in LDS
constexpr int VROWS = 8;                                 // output rows per lane of the vertical pass: lanes 0..191 = 2 x (TX * 3 byte columns)
// the widest tile: TX - 1 steps of at most 64 (1 + 2^-40) px between the first and the last window, one window, and the dword slack
static_assert(3 * ((TX - 1) * 65 + MAX_TAPS + 1) + 6 <= SRC_BYTES, "one source row of a tile must fit the LDS chunk");
static_assert(TX * 3 * (TY / VROWS) <= 256 && ROWS * TX == 256 && TY % VROWS == 0, "lane roles");

struct Axis { double in0, scale, fs; };

// in0 = 0.5 - (t + 0.5) / s, in1 = in0 + size / s, scale = (in1 - in0) / size, fs = max(scale, 1)
__device__ __forceinline__ Axis area_axis(double s, double t, int size) {
#pragma clang fp contract(off)
    Axis ax;
    ax.in0 = 0.5 - (t + 0.5) / s;
    const double in1 = ax.in0 + (double)size / s;
    ax.scale = (in1 - ax.in0) / (double)size;
    ax.fs = ax.scale > 1. ? ax.scale : 1.;
    return ax;
}

__device__ __forceinline__ double tap_weight(int x, double c, double fs) {
#pragma clang fp contract(off)
    const double w = 1. - fabs(((double)x - c + 0.5) / fs);
    return w > 0. ? w : 0.;
}

// output position u of one axis -> first tap, tap count, and the taps' weights K[0 .. n) = (int)(k / sum(k) * 2^22 + 0.5); the sum runs in tap order
__device__ __forceinline__ void area_coeffs(const Axis& ax, int u, int* K, int& first, int& n) {
#pragma clang fp contract(off)
    const double c = ax.in0 + ((double)u + 0.5) * ax.scale;
    first = (int)floor(c - ax.fs + 0.5);
    n = (int)floor(c + ax.fs + 0.5) - first;
    n = n < 0 ? 0 : (n > MAX_TAPS ? MAX_TAPS : n);       // fs <= 64 (1 + 2^-40) gives at most 129 taps; the clamp keeps the LDS row whatever the input
    double ww = 0.;
    for (int j = 0; j < n; ++j) ww += tap_weight(first + j, c, ax.fs);
    for (int j = 0; j < n; ++j) K[j] = (int)(tap_weight(first + j, c, ax.fs) / ww * (double)(1 << PREC) + 0.5);
}

__device__ __forceinline__ int clip8(int acc) {
    const int v = (acc + (1 << (PREC - 1))) >> PREC;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

__global__ __launch_bounds__(256) void area_kernel(CropArgs a) {
    __shared__ int Kx[TX][MAX_TAPS], Ky[TY][MAX_TAPS];
    __shared__ int x_first[TX], x_n[TX], y_first[TY], y_n[TY];
    __shared__ unsigned src[SRC_BYTES / 4];
    __shared__ unsigned char tmp[ROWS][TX * 3];
    const int b = blockIdx.z, x0 = blockIdx.x * TX, y0 = blockIdx.y * TY, tid = threadIdx.x, size = a.size;
    Image im;
    load_image(a, b, im);
    if (!area_rule(a, b, im)) return;                    // the whole workgroup: crop_kernel<true> made (or blackened) this image
    const int nx = size - x0 < TX ? size - x0 : TX, ny = size - y0 < TY ? size - y0 : TY;      // the tile's columns and rows inside the crop

    // coefficients: lanes 0..31 the columns, lanes 64..79 the rows (another wave)
    {
        const double* M = a.M + (long long)b * 6;
        if (tid < TX) {
            int first = 0, n = 0;
            if (tid < nx) area_coeffs(area_axis(M[0], M[2], size), x0 + tid, Kx[tid], first, n);
            x_first[tid] = first; x_n[tid] = n;
        } else if (tid >= 64 && tid < 64 + TY) {
            const int t = tid - 64;
            int first = 0, n = 0;
            if (t < ny) area_coeffs(area_axis(M[4], M[5], size), y0 + t, Ky[t], first, n);
            y_first[t] = first; y_n[t] = n;
        }
    }
    __syncthreads();

    // the part of the frame the tile reads; first tap and last tap grow with the output position.  Outside the frame nothing is loaded
    const int clo = x_first[0] > 0 ? x_first[0] : 0;
    const int cend = x_first[nx - 1] + x_n[nx - 1], chi = cend < im.w ? cend : im.w;
    const int rlo = y_first[0] > 0 ? y_first[0] : 0;
    const int rend = y_first[ny - 1] + y_n[ny - 1], rhi = rend < im.h ? rend : im.h;
    const int nbytes = chi > clo ? (chi - clo) * 3 : 0;
    const int nd = (nbytes + 6) >> 2;                    // dwords per staged row: its first byte may sit 3 bytes into the first dword
    int R = nd ? (SRC_BYTES / 4) / nd : ROWS;            // >= 2 by the static_assert above
    R = R > ROWS ? ROWS : R;

    const int hx = tid % TX, hr = tid / TX;              // horizontal pass: lane = (row of the chunk, column of the tile)
    const int ve = tid % (TX * 3), vg = tid / (TX * 3);  // vertical pass: lane = (byte column of the tile, group of VROWS output rows)
    const bool vlane = vg < TY / VROWS && ve < nx * 3;
    int vfirst[VROWS], vn[VROWS], acc[VROWS];
#pragma unroll
    for (int i = 0; i < VROWS; ++i) {
        const int t = vg * VROWS + i;
        vfirst[i] = vlane && t < ny ? y_first[t] : 0;
        vn[i] = vlane && t < ny ? y_n[t] : 0;
        acc[i] = 0;
    }
    const int hfirst = x_first[hx], hn = hx < nx ? x_n[hx] : 0;
    const int j0 = hfirst < 0 ? -hfirst : 0, j1 = hn < im.w - hfirst ? hn : im.w - hfirst;      // the taps inside the frame
    const uintptr_t lo = (uintptr_t)a.frames, hi = lo + (uintptr_t)a.bytes;

    for (int r0 = rlo; r0 < rhi && nbytes; r0 += R) {
        const int nr = rhi - r0 < R ? rhi - r0 : R;
        // stage rows r0 .. r0 + nr, columns clo .. chi: aligned dwords from the dword that holds the row's first byte
        for (int idx = tid; idx < nr * nd; idx += 256) {
            const int rr = (int)((unsigned)idx / (unsigned)nd), i = idx - rr * nd;
            const uintptr_t p = (((uintptr_t)im.f + (uintptr_t)((long long)(r0 + rr) * im.stride + 3ll * clo)) & ~(uintptr_t)3) + 4u * (unsigned)i;
            unsigned v = 0u;
            if (p >= lo && p + 4 <= hi) {
                v = *reinterpret_cast<const unsigned*>(p);
            } else {                                     // a dword across an end of the buffer: its bytes inside, one by one
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (p + k >= lo && p + k < hi) v |= (unsigned)*reinterpret_cast<const unsigned char*>(p + k) << (8 * k);
            }
            src[idx] = v;
        }
        __syncthreads();
        if (hr < nr && hx < nx) {
            const unsigned shift = (unsigned)(((uintptr_t)im.f + (uintptr_t)((long long)(r0 + hr) * im.stride + 3ll * clo)) & 3u);
            const unsigned char* s = reinterpret_cast<const unsigned char*>(src);
            const int at = hr * nd * 4 + (int)shift + (hfirst - clo) * 3;             // byte of tap 0 (before the row where tap 0 is outside the frame)
            int h0 = 0, h1 = 0, h2 = 0;
            for (int j = j0; j < j1; ++j) {
                const int k = Kx[hx][j], o = at + j * 3;
                h0 += k * (int)s[o + 0]; h1 += k * (int)s[o + 1]; h2 += k * (int)s[o + 2];
            }
            tmp[hr][hx * 3 + 0] = (unsigned char)clip8(h0);
            tmp[hr][hx * 3 + 1] = (unsigned char)clip8(h1);
            tmp[hr][hx * 3 + 2] = (unsigned char)clip8(h2);
        }
        __syncthreads();
        if (vlane) {
            for (int rr = 0; rr < nr; ++rr) {
                const int v = tmp[rr][ve], row = r0 + rr;
#pragma unroll
                for (int i = 0; i < VROWS; ++i) {
                    const int d = row - vfirst[i];
                    if ((unsigned)d < (unsigned)vn[i]) acc[i] += Ky[vg * VROWS + i][d] * v;
                }
            }
        }
        // the next chunk's staging writes src only; its barrier comes before tmp is written again
    }
    if (vlane) {
#pragma unroll
        for (int i = 0; i < VROWS; ++i) {
            const int t = vg * VROWS + i;
            if (t < ny) a.out[(((long long)b * size + (y0 + t)) * size + x0) * 3 + ve] = (unsigned char)clip8(acc[i]);
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
    a.frames = frames; a.bytes = frames_bytes; a.descs = descs; a.M = M; a.valid = valid; a.out = out; a.status = status; a.area = nullptr; a.B = B; a.size = size;
    const long long lanes = ((long long)B * size * size + PIX - 1) / PIX;
    DIR_LAUNCH((crop_kernel<false>), dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    return dir::check_launch("dir_crop_frames");
}

extern "C" int dir_crop_frames_area(const uint8_t* frames, long long frames_bytes, const dir_frame_desc* descs, const double* M, const int32_t* valid,
                                    int B, int size, uint8_t* out, int32_t* status, int32_t* area, void* stream) {
    if (B == 0) return DIR_OK;
    DIR_REQUIRE(frames && descs && M && out, "dir_crop_frames_area: null pointer");
    DIR_REQUIRE(crop_common_ok(B, 1., size) && frames_bytes > 0, "dir_crop_frames_area: bad args (B %d outside 1..%d, size %d outside %d..%d or %lld bytes of frames)",
                B, DIR_CROP_MAX_BATCH, size, DIR_CROP_MIN_SIZE, DIR_CROP_MAX_SIZE, frames_bytes);
    DIR_REQUIRE(((uintptr_t)out & 3) == 0, "dir_crop_frames_area: out must be 4-byte aligned");
    CropArgs a;
    a.frames = frames; a.bytes = frames_bytes; a.descs = descs; a.M = M; a.valid = valid; a.out = out; a.status = status; a.area = area; a.B = B; a.size = size;
    // two launches that write disjoint bytes: the plain rule (and every black crop, status and area flag), then the shrinking images
    const long long lanes = ((long long)B * size * size + PIX - 1) / PIX;
    DIR_LAUNCH((crop_kernel<true>), dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    DIR_LAUNCH(area_kernel, dim3((size + TX - 1) / TX, (size + TY - 1) / TY, B), dim3(256), 0, (hipStream_t)stream, a);
    return dir::check_launch("dir_crop_frames_area");
}
