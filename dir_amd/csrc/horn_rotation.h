// Horn 1987: the proper rotation that best maps one point set onto another, from their 3 x 3 cross-covariance, by cyclic Jacobi sweeps on the
// symmetric 4 x 4 quaternion matrix.  Two kernels call it: procrustes_kernel (alignmetric.hip, whose header comment states the rule) and
// mano_fit_start_kernel (mano_fit_start.hip).  One thread, registers only: every index is a compile-time constant.
#pragma once
#include "dir_common.h"

namespace dir {

constexpr int JACOBI_SWEEPS = 12;      // 5 suffice on every input tried; the loop leaves when the off-diagonal is exactly 0

// one Jacobi rotation of the symmetric a (and of the eigenvector columns v) that zeroes a[P][Q]; Numerical Recipes' update formulas
template <int P, int Q> __device__ __forceinline__ void jacobi_rotate(float (&a)[4][4], float (&v)[4][4]) {
    const float apq = a[P][Q];
    if (apq == 0.f) return;
    const float theta = (a[Q][Q] - a[P][P]) / (2.f * apq);
    // the smaller root of t^2 + 2 t theta - 1 = 0; an overflowing theta gives t = 0, which is its value to float32
    const float t = copysignf(1.f, theta) / (fabsf(theta) + sqrtf(theta * theta + 1.f));
    const float c = 1.f / sqrtf(t * t + 1.f), s = t * c, tau = s / (1.f + c);
    a[P][P] -= t * apq, a[Q][Q] += t * apq, a[P][Q] = 0.f, a[Q][P] = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (r != P && r != Q) {
            const float g = a[r][P], h = a[r][Q];
            a[r][P] = a[P][r] = g - s * (h + g * tau);
            a[r][Q] = a[Q][r] = h + s * (g - h * tau);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float g = v[r][P], h = v[r][Q];
        v[r][P] = g - s * (h + g * tau);
        v[r][Q] = h + s * (g - h * tau);
    }
}

// S[a][b] = sum p_a g_b -> the proper rotation R (row-major) that maximises sum g . R p
__device__ inline void horn_rotation(const float (&S)[9], float (&R)[9]) {
    const float Sxx = S[0], Sxy = S[1], Sxz = S[2], Syx = S[3], Syy = S[4], Syz = S[5], Szx = S[6], Szy = S[7], Szz = S[8];
    float a[4][4] = {{Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx},
                     {Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz},
                     {Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy},
                     {Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz}};
    float v[4][4] = {{1.f, 0.f, 0.f, 0.f}, {0.f, 1.f, 0.f, 0.f}, {0.f, 0.f, 1.f, 0.f}, {0.f, 0.f, 0.f, 1.f}};
    float m = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) m = fmaxf(m, fabsf(a[i][j]));
    if (m > 0.f) {
        const float inv = 1.f / m;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) a[i][j] *= inv;
    }
    for (int sweep = 0; sweep < JACOBI_SWEEPS; ++sweep) {
        const float off = fabsf(a[0][1]) + fabsf(a[0][2]) + fabsf(a[0][3]) + fabsf(a[1][2]) + fabsf(a[1][3]) + fabsf(a[2][3]);
        if (off == 0.f) break;
        jacobi_rotate<0, 1>(a, v), jacobi_rotate<0, 2>(a, v), jacobi_rotate<0, 3>(a, v);
        jacobi_rotate<1, 2>(a, v), jacobi_rotate<1, 3>(a, v), jacobi_rotate<2, 3>(a, v);
    }
    // the eigenvector of the largest eigenvalue (the first of equal ones), by selects: no runtime index
    float best = a[0][0], w = v[0][0], x = v[1][0], y = v[2][0], z = v[3][0];
#pragma unroll
    for (int k = 1; k < 4; ++k) {
        const bool take = a[k][k] > best;
        best = take ? a[k][k] : best;
        w = take ? v[0][k] : w, x = take ? v[1][k] : x, y = take ? v[2][k] : y, z = take ? v[3][k] : z;
    }
    const float n = 1.f / sqrtf(w * w + x * x + y * y + z * z);
    w *= n, x *= n, y *= n, z *= n;
    R[0] = 1.f - 2.f * (y * y + z * z), R[1] = 2.f * (x * y - w * z), R[2] = 2.f * (x * z + w * y);
    R[3] = 2.f * (x * y + w * z), R[4] = 1.f - 2.f * (x * x + z * z), R[5] = 2.f * (y * z - w * x);
    R[6] = 2.f * (x * z - w * y), R[7] = 2.f * (y * z + w * x), R[8] = 1.f - 2.f * (x * x + y * y);
}

}  // namespace dir
