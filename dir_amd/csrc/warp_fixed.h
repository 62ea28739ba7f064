// The coordinate rules of cv.warpAffine for 8-bit images, INTER_LINEAR (imgwarp.cpp WarpAffineInvoker + remapBilinear), shared by
// csrc/augment.hip (256 x 256 sources) and csrc/crop.hip (sources of any size).  Restated in numpy by tests/helpers/augment_ref.py.
// Every function switches floating-point contraction off: the products and sums are rounded one by one, as OpenCV's are.
#pragma once
#include <hip/hip_runtime.h>

namespace warp {

constexpr int AB_BITS = 10, AB_SCALE = 1 << AB_BITS, INTER_BITS = 5, INTER_TAB = 1 << INTER_BITS;
constexpr int ROUND_DELTA = AB_SCALE / INTER_TAB / 2;     // 16: INTER_LINEAR's rounding of the 10-bit coordinate to 5 bits
constexpr int COEF_BITS = 15;                             // INTER_REMAP_COEF_BITS: the four weights sum to 32768

// cv::invertAffineTransform in double, on a float32 or double 2x3 matrix
template <typename T> __device__ __forceinline__ void invert_affine(const T* Mf, double* m) {
#pragma clang fp contract(off)
    const double M0 = Mf[0], M1 = Mf[1], M2 = Mf[2], M3 = Mf[3], M4 = Mf[4], M5 = Mf[5];
    double D = M0 * M4 - M1 * M3;
    D = D != 0. ? 1. / D : 0.;
    m[0] = M4 * D;
    m[1] = M1 * -D;
    m[3] = M3 * -D;
    m[4] = M0 * D;
    m[2] = -m[0] * M2 - m[1] * M5;
    m[5] = -m[3] * M2 - m[4] * M5;
}

// source position of output pixel (x, y): integer part (sx, sy) and 5-bit fractions (fx, fy) -- AB_BITS = 10 fixed point per row and column
// (saturate_cast<int> = round half to even), summed, then rounded to INTER_BITS
__device__ __forceinline__ void warp_coord(const double* m, int x, int y, int& sx, int& sy, int& fx, int& fy) {
#pragma clang fp contract(off)
    const int X0 = (int)rint((m[1] * (double)y + m[2]) * (double)AB_SCALE) + ROUND_DELTA;
    const int Y0 = (int)rint((m[4] * (double)y + m[5]) * (double)AB_SCALE) + ROUND_DELTA;
    const int ad = (int)rint(m[0] * (double)x * (double)AB_SCALE);
    const int bd = (int)rint(m[3] * (double)x * (double)AB_SCALE);
    const int X = (X0 + ad) >> (AB_BITS - INTER_BITS), Y = (Y0 + bd) >> (AB_BITS - INTER_BITS);
    sx = X >> INTER_BITS; sy = Y >> INTER_BITS;
    fx = X & (INTER_TAB - 1); fy = Y & (INTER_TAB - 1);
}

// the four 15-bit bilinear weights of the taps (0,0), (1,0), (0,1), (1,1)
__device__ __forceinline__ void warp_weights(int fx, int fy, int* w) {
    w[0] = (INTER_TAB - fy) * (INTER_TAB - fx) * INTER_TAB;
    w[1] = (INTER_TAB - fy) * fx * INTER_TAB;
    w[2] = fy * (INTER_TAB - fx) * INTER_TAB;
    w[3] = fy * fx * INTER_TAB;
}

// (sum + 2^14) >> 15, clamped to a byte
__device__ __forceinline__ int warp_round(int acc) {
    const int v = (acc + (1 << (COEF_BITS - 1))) >> COEF_BITS;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

}  // namespace warp
