// Train-split input of dataset/interhand.py:__getitem__ (split 'train') for a whole batch on the GPU: flip, motion blur, affine warp,
// seg from the warped mask, add_noise, the normalised image and the label maths (utils/utils.py:202-207, 406-533).
//
//   blur_kernel    utils.py:526-533 cv.filter2D(img, -1, k) of the images drawn for blur, into a scratch frame (flipped frame coordinates)
//   image_kernel   flip + cv.warpAffine(INTER_LINEAR, BORDER_CONSTANT 0) of img / mask / dense, seg (interhand.py:206-216), add_noise
//                  (utils.py:446-452) and the outputs of interhand.py:218-228
//   label_kernel   flip (utils.py:476-493, interhand.py:170-182), the 2x3 affine on uv, uvd2xyz_np, (uv/256*2-1, z) and center_*
//
// The fixed-point rules are the published OpenCV algorithm (imgwarp.cpp WarpAffineInvoker + remapBilinear for 8-bit images, filter.cpp
// Filter2D); they are restated in numpy in tests/helpers/augment_ref.py and are unpinned against the library itself, which is not available.
#include "dir_common.h"
#include "warp_fixed.h"

namespace {

using namespace warp;      // the fixed-point coordinate rules, shared with csrc/crop.hip

constexpr int S = 256, HW = S * S;
constexpr int NJ = 21, NV = 778, NP = NJ + NV;

struct NormArgs { float mean[3], stdv[3]; };

// bilinear tap of one channel; a tap outside the frame reads 0 (BORDER_CONSTANT per tap); `flip` mirrors the source columns
__device__ __forceinline__ int bilinear_u8(const unsigned char* f, int sx, int sy, const int* w, int c, int flip) {
    int acc = 0;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int xx = sx + (t & 1), yy = sy + (t >> 1);
        if ((unsigned)xx < (unsigned)S && (unsigned)yy < (unsigned)S) acc += (int)f[((yy * S) + (flip ? S - 1 - xx : xx)) * 3 + c] * w[t];
    }
    const int v = (acc + (1 << (COEF_BITS - 1))) >> COEF_BITS;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

__device__ __forceinline__ unsigned long long splitmix64(unsigned long long z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// 255 * N(0, 0.01) for element (image b, pixel p, channel c); see dir_train_noise_field in include/dir_hip.h
__device__ __forceinline__ float gauss_255(unsigned long long seed, int b, int p, int c) {
#pragma clang fp contract(off)
    const unsigned long long h = splitmix64(splitmix64(seed) + ((unsigned long long)b * HW + (unsigned long long)p) * 3ull + (unsigned long long)c);
    const float u1 = ((float)(h >> 41) + 0.5f) * 0x1p-23f;                 // (0, 1)
    const float u2 = (float)(h & 0xFFFFFFull) * 0x1p-24f;                 // [0, 1)
    return 2.55f * (sqrtf(-2.f * logf(u1)) * cosf(6.28318530717958647692f * u2));
}

__device__ __forceinline__ float norm_px(unsigned char v, float mean, float stdv) {
#pragma clang fp contract(off)
    return ((float)v / 255.f - mean) / stdv;                               // == dir_image_normalize_forward (csrc/spatial.hip)
}

__device__ __forceinline__ int reflect101(int p) { return p < 0 ? -p : (p >= S ? 2 * S - 2 - p : p); }

// filter2D with reflect-101 borders, of the FLIPPED frame (the reference blurs after flipping); written in flipped coordinates
__global__ __launch_bounds__(256) void blur_kernel(const dir_aug_params* __restrict__ P, const unsigned char* __restrict__ img,
                                                   unsigned char* __restrict__ out, int B) {
#pragma clang fp contract(off)
    const long long i = blockIdx.x * 256ll + threadIdx.x;                  // a 256-thread block never spans two images
    const int b = (int)(i / HW), p = (int)(i - (long long)b * HW);
    if (b >= B) return;
    const int ks = P[b].blur;
    if (ks < 1 || ks > DIR_AUG_MAX_BLUR) return;
    const int flip = P[b].flip, anchor = ks / 2, y = p / S, x = p - y * S;
    const unsigned char* f = img + (long long)b * HW * 3;
    float acc[3] = {0.f, 0.f, 0.f};
    for (int r = 0; r < ks; ++r) {
        const int yy = reflect101(y + r - anchor);
        for (int q = 0; q < ks; ++q) {
            const int xf = reflect101(x + q - anchor);
            const float k = P[b].kernel[r * ks + q];
            const unsigned char* px = f + (yy * S + (flip ? S - 1 - xf : xf)) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c] = acc[c] + k * (float)px[c];
        }
    }
    unsigned char* o = out + i * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int v = (int)rintf(acc[c]);                                  // saturate_cast<uchar>(float): round half to even, clamp
        o[c] = (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
    }
}

struct ImageArgs {
    const dir_aug_params* P;
    const unsigned char *img, *mask, *dense, *blurred;
    const float* noise;
    unsigned long long seed;
    float *img_nchw, *img_rgb, *mask_rgb, *seg, *dense_out;
    int B;
    NormArgs nm;
};

__global__ __launch_bounds__(256) void image_kernel(ImageArgs a) {
#pragma clang fp contract(off)
    const long long i = blockIdx.x * 256ll + threadIdx.x;
    const int b = (int)(i / HW), p = (int)(i - (long long)b * HW);
    if (b >= a.B) return;
    const dir_aug_params& P = a.P[b];
    const int y = p / S, x = p - y * S, flip = P.flip != 0;
    const bool blurred = P.blur >= 1 && P.blur <= DIR_AUG_MAX_BLUR;
    double m[6];
    invert_affine(P.M, m);
    int sx, sy, fx, fy;
    warp_coord(m, x, y, sx, sy, fx, fy);
    const int w[4] = {(INTER_TAB - fy) * (INTER_TAB - fx) * INTER_TAB, (INTER_TAB - fy) * fx * INTER_TAB, fy * (INTER_TAB - fx) * INTER_TAB,
                      fy * fx * INTER_TAB};
    const long long fo = (long long)b * HW * 3;
    unsigned char im[3], mk[3], dn[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        im[c] = (unsigned char)(blurred ? bilinear_u8(a.blurred + fo, sx, sy, w, c, 0) : bilinear_u8(a.img + fo, sx, sy, w, c, flip));
        mk[c] = (unsigned char)bilinear_u8(a.mask + fo, sx, sy, w, c, flip);
        dn[c] = (unsigned char)bilinear_u8(a.dense + fo, sx, sy, w, c, flip);
    }
    // seg: hand = G > 50 | R > 50; left = hand & G >= R, right = hand & G < R; labels 1 / 2, swapped when flipped
    const bool hand = mk[1] > 50 || mk[2] > 50;
    const float left = flip ? 2.f : 1.f, right = flip ? 1.f : 2.f;
    a.seg[(long long)b * HW + p] = !hand ? 0.f : (mk[1] >= mk[2] ? left : right);
    // add_noise in fp64: a * img + b + 255 * N(0, 0.01), clip(0, 255), astype(uint8) truncates
    unsigned char nz[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float n = a.noise ? a.noise[fo + (long long)p * 3 + c] : gauss_255(a.seed, b, p, c);
        double v = P.a[c] * (double)im[c] + P.b + (double)n;
        v = v > 0. ? (v < 255. ? v : 255.) : 0.;
        nz[c] = (unsigned char)(int)v;
    }
    const long long po = fo + (long long)p * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (a.img_rgb) a.img_rgb[po + c] = (float)nz[c];
        if (a.mask_rgb) a.mask_rgb[po + c] = (float)mk[c];
        a.img_nchw[((long long)b * 3 + c) * HW + p] = norm_px(nz[2 - c], a.nm.mean[c], a.nm.stdv[c]);
        a.dense_out[((long long)b * 3 + c) * HW + p] = (float)dn[c] / 255.f;
    }
}

__global__ __launch_bounds__(256) void noise_kernel(unsigned long long seed, float* __restrict__ out, int B) {
    const long long i = blockIdx.x * 256ll + threadIdx.x;
    const int b = (int)(i / HW), p = (int)(i - (long long)b * HW);
    if (b >= B) return;
#pragma unroll
    for (int c = 0; c < 3; ++c) out[i * 3 + c] = gauss_255(seed, b, p, c);
}

struct LabelArgs {
    const dir_aug_params* P;
    const float* in[8];      // joint_xyz L, mesh_xyz L, joint_xyz R, mesh_xyz R, joint_uv L, mesh_uv L, joint_uv R, mesh_uv R
    const float* cam;
    float* out[10];          // joint_2d L, mesh_2d L, joint_2d R, mesh_2d R, joint_3d L, mesh_3d L, joint_3d R, mesh_3d R, center L, center R
    int B;
};

__global__ __launch_bounds__(256) void label_kernel(LabelArgs a) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.B * 2 * NP) return;
    const int b = i / (2 * NP), r = i - b * 2 * NP, h = r / NP, q = r - h * NP;
    const bool joint = q < NJ;
    const int k = joint ? q : q - NJ, n = joint ? NJ : NV, kind = joint ? 0 : 1;
    const int flip = a.P ? a.P[b].flip != 0 : 0;
    const int hs = flip ? 1 - h : h;                                       // left / right swap of the labels when flipped
    const long long e = (long long)b * n + k;
    const float* xyz = a.in[kind + 2 * hs] + e * 3;
    const float* uv = a.in[4 + kind + 2 * hs] + e * 2;
    double u = uv[0], v = uv[1], X = xyz[0], Y = xyz[1];
    const double Z = xyz[2];
    if (a.P) {
        const float* M = a.P[b].M;
        const float* K = a.cam + (long long)b * 9;
        if (flip) u = ((double)S - u) - 1.;
        const double u2 = u * (double)M[0] + v * (double)M[1] + (double)M[2];
        const double v2 = u * (double)M[3] + v * (double)M[4] + (double)M[5];
        u = u2; v = v2;
        X = (u - (double)K[2]) * Z / (double)K[0];                         // uvd2xyz_np
        Y = (v - (double)K[5]) * Z / (double)K[4];
    }
    float* o2 = a.out[kind + 2 * h] + e * 3;
    float* o3 = a.out[4 + kind + 2 * h] + e * 3;
    o2[0] = (float)(u / (double)S * 2. - 1.);
    o2[1] = (float)(v / (double)S * 2. - 1.);
    o2[2] = (float)Z;
    o3[0] = (float)X; o3[1] = (float)Y; o3[2] = (float)Z;
    if (joint && k == 9) {
        float* oc = a.out[8 + h] + (long long)b * 3;
        oc[0] = (float)X; oc[1] = (float)Y; oc[2] = (float)Z;
    }
}

}  // namespace

extern "C" int dir_train_noise_field(unsigned long long seed, float* out, int B, void* stream) {
    if (B == 0) return DIR_OK;
    DIR_REQUIRE(out && B > 0 && B <= DIR_AUG_MAX_BATCH, "dir_train_noise_field: bad args (out %p, B %d)", (void*)out, B);
    DIR_LAUNCH(noise_kernel, dim3(B * (HW / 256)), dim3(256), 0, (hipStream_t)stream, seed, out, B);
    return dir::check_launch("dir_train_noise_field");
}

extern "C" int dir_train_augment_images(const dir_aug_params* params, const uint8_t* img, const uint8_t* mask, const uint8_t* dense,
                                        const float* noise, unsigned long long seed, const float* mean_host, const float* std_host,
                                        uint8_t* blur_scratch, float* img_nchw, float* img_rgb, float* mask_rgb, float* seg,
                                        float* dense_out, int B, void* stream) {
    if (B == 0) return DIR_OK;
    DIR_REQUIRE(params && img && mask && dense && blur_scratch && img_nchw && seg && dense_out && B > 0 && B <= DIR_AUG_MAX_BATCH,
                "dir_train_augment_images: bad args (null pointer or B %d outside 1..%d)", B, DIR_AUG_MAX_BATCH);
    DIR_REQUIRE(mean_host && std_host, "dir_train_augment_images: null mean / std (host pointers to 3 floats)");
    ImageArgs a;
    for (int c = 0; c < 3; ++c) {
        DIR_REQUIRE(std_host[c] != 0.f, "dir_train_augment_images: std[%d] is zero", c);
        a.nm.mean[c] = mean_host[c];
        a.nm.stdv[c] = std_host[c];
    }
    a.P = params; a.img = img; a.mask = mask; a.dense = dense; a.blurred = blur_scratch; a.noise = noise; a.seed = seed;
    a.img_nchw = img_nchw; a.img_rgb = img_rgb; a.mask_rgb = mask_rgb; a.seg = seg; a.dense_out = dense_out; a.B = B;
    hipStream_t s = (hipStream_t)stream;
    DIR_LAUNCH(blur_kernel, dim3(B * (HW / 256)), dim3(256), 0, s, params, img, blur_scratch, B);
    if (int rc = dir::check_launch("dir_train_augment_images (blur)")) return rc;
    DIR_LAUNCH(image_kernel, dim3(B * (HW / 256)), dim3(256), 0, s, a);
    return dir::check_launch("dir_train_augment_images");
}

extern "C" int dir_train_augment_labels(const dir_aug_params* params, const float* const* in_host, const float* camera, float* const* out_host,
                                        int B, void* stream) {
    if (B == 0) return DIR_OK;
    DIR_REQUIRE(in_host && out_host && B > 0 && B <= DIR_AUG_MAX_BATCH, "dir_train_augment_labels: bad args (B %d)", B);
    DIR_REQUIRE(camera || !params, "dir_train_augment_labels: camera is needed with params");
    LabelArgs a;
    a.P = params; a.cam = camera; a.B = B;
    for (int j = 0; j < 8; ++j) {
        DIR_REQUIRE(in_host[j], "dir_train_augment_labels: input %d is null", j);
        a.in[j] = in_host[j];
    }
    for (int j = 0; j < 10; ++j) {
        DIR_REQUIRE(out_host[j], "dir_train_augment_labels: output %d is null", j);
        a.out[j] = out_host[j];
    }
    const int n = B * 2 * NP;
    DIR_LAUNCH(label_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, a);
    return dir::check_launch("dir_train_augment_labels");
}
