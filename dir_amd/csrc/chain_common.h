// Device pieces shared by the persistent 8-wave "chain" kernels (bneck.hip, tail.hip, l3_chain.hip, res_chain.hip).  gfx950 only.
// Every GEMM of these kernels is D[channel][pixel] on v_mfma_f32_32x32x16 (or 16x16x32): of a 32-channel block a lane holds, per q = 0 .. 3,
// accumulator elements 4 q .. 4 q + 3 = channels 8 q + 4 h .. + 4 (h = lane >> 5) of pixel l32 = lane & 31 -- four consecutive stored channels,
// one uint2.  What follows is that layout's epilogue arithmetic, its 16-byte global accesses, and the tile order of the persistent grid.
//
// The callers sit at the register limit (tail_chain, tail_thin and l3_chain<256> use all 256 VGPRs), where the allocation follows the order and
// form of the IR, not only its meaning.  Every piece here was checked to leave each caller's resource figures and instruction counts as they were
// with the code written out (tools/kernel_resources.py --diff, profiles/chain_common_resources.txt); that is why scalars arrive by const
// reference (a by-value copy moved spill counts), and why store_t_to_out takes s_t and c4 by value (by reference they did).  Check again after
// any edit.  Epilogue C of the 32x32 path (bn1 + ReLU -> y1n) is NOT here: as one function it changed tail_chain_kernel<256, 256>'s spills in
// every form tried; tail.hip and l3_chain.hip each build it from bn_relu4 and store16_swapped.
#pragma once
#include "conv_common.h"

namespace dir {
namespace chain {

using convk::bf16_t;
using convk::f32x16;
using convk::Half;

template <int V> struct IC : std::integral_constant<int, V> {};      // a compile-time index as a lambda argument

template <typename H> __device__ __forceinline__ void unpack4(uint2 v, float (&f)[4]) {
    convk::unpack2<H>(v.x, f[0], f[1]);
    convk::unpack2<H>(v.y, f[2], f[3]);
}

// BatchNorm (folded scale / shift) + ReLU of accumulator elements 4 q .. 4 q + 3, rounded to the storage kind H
template <typename H, typename Acc>
__device__ __forceinline__ uint2 bn_relu4(const Acc& acc, const int& q, const float4& sc, const float4& sh) {
    return make_uint2(Half<H>::pack2_relu(fmaf(acc[4 * q], sc.x, sh.x), fmaf(acc[4 * q + 1], sc.y, sh.y)),
                      Half<H>::pack2_relu(fmaf(acc[4 * q + 2], sc.z, sh.z), fmaf(acc[4 * q + 3], sc.w, sh.w)));
}
// ... in two steps where an identity is added before the ReLU: v = bn, then round(relu(v + rv)).  (Two steps, so that callers keep the order
// fmaf -> fetch the identity -> four adds -> two packs of the code these came from: with the adds inside the pack expressions the epilogues were
// scheduled differently and tail_chain<128, 128> measured 1 % slower.)
template <typename Acc>
__device__ __forceinline__ void bn4(const Acc& acc, const int& q, const float4& sc, const float4& sh, float (&v)[4]) {
    v[0] = fmaf(acc[4 * q], sc.x, sh.x); v[1] = fmaf(acc[4 * q + 1], sc.y, sh.y); v[2] = fmaf(acc[4 * q + 2], sc.z, sh.z); v[3] = fmaf(acc[4 * q + 3], sc.w, sh.w);
}
template <typename H> __device__ __forceinline__ uint2 add_relu4(const float (&v)[4], const float (&rv)[4]) {
    float s[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) s[e] = v[e] + rv[e];
    return make_uint2(Half<H>::pack2_relu(s[0], s[1]), Half<H>::pack2_relu(s[2], s[3]));
}

// The identity of a 32-channel block of one pixel as two 16-byte chunks: rp = the pixel's block + 8 h, so lane half h holds channels
// 16 j + 8 h .. + 8 in x[j] -- half the load instructions of 8-byte pieces in the accumulator layout, 32 contiguous bytes per pixel row
__device__ __forceinline__ void res16_fetch(const bf16_t* const& rp, uint4 (&x)[2]) {
#pragma unroll
    for (int j = 0; j < 2; ++j) x[j] = *reinterpret_cast<const uint4*>(rp + 16 * j);
}
// ... and its channels of accumulator group q: (q even, q odd) = swap(lower 8 bytes, upper 8 bytes) of chunk q / 2 with the partner lane
// (v_permlane32_swap), dword by dword
template <typename H> __device__ __forceinline__ void res16_take(const uint4 (&x)[2], const int& q, float (&rv)[4]) {
    const uint4 c = x[q >> 1];
    const auto sx = __builtin_amdgcn_permlane32_swap(c.x, c.z, false, false);
    const auto sy = __builtin_amdgcn_permlane32_swap(c.y, c.w, false, false);
    unpack4<H>(make_uint2(sx[q & 1], sy[q & 1]), rv);
}
// The swap in reverse: o[q] = the lane's four channels of group q; lane half h leaves with channels 16 j + 8 h .. + 8 -- one 16-byte store
// per j at p = the pixel's block + 8 h
__device__ __forceinline__ void store16_swapped(const uint2 (&o)[4], bf16_t* const& p) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const auto dx = __builtin_amdgcn_permlane32_swap(o[2 * j].x, o[2 * j + 1].x, false, false);
        const auto dy = __builtin_amdgcn_permlane32_swap(o[2 * j].y, o[2 * j + 1].y, false, false);
        *reinterpret_cast<uint4*>(p + 16 * j) = make_uint4(dx[0], dy[0], dx[1], dy[1]);
    }
}

// Epilogue B of one 32-channel block (conv3 of tail.hip / l3_chain.hip): bn3 + identity + ReLU -> T tile in LDS, rounded -- the rounding point
// of the stored block output.  accb / xr: [pixel block pb]; s_sc, s_sh: the half's vectors; cbase: the block's first channel inside the half
template <typename H, int TPITCH>
__device__ __forceinline__ void epilogue_b(const f32x16 (&accb)[2], const uint4 (&xr)[2][2], const float* const& s_sc, const float* const& s_sh, char* const& s_t,
                                           const int& cbase, const int& l32, const int& h) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int cl = cbase + 8 * q + 4 * h;
        const float4 sc = *reinterpret_cast<const float4*>(s_sc + cl);
        const float4 sh = *reinterpret_cast<const float4*>(s_sh + cl);
#pragma unroll
        for (int pb = 0; pb < 2; ++pb) {
            float v[4], rv[4];
            bn4(accb[pb], q, sc, sh, v);
            res16_take<H>(xr[pb], q, rv);
            *reinterpret_cast<uint2*>(s_t + (32 * pb + l32) * TPITCH + cl * 2) = add_relu4<H>(v, rv);
        }
        __builtin_amdgcn_sched_barrier(0);          // keep the (sc, sh) reads of later q's out of this one's registers
    }
}

// Block output: T ([TM pixels][HC channels], TPITCH bytes per pixel) -> out rows of c4 channels, coalesced 16-byte stores (chunk c = pixel
// c / (HC / 8), 16-byte chunk c % (HC / 8)) of tile t, half hf
template <int NTHR, int TM, int HC, int TPITCH>
__device__ __forceinline__ void store_t_to_out(const char* s_t, bf16_t* const& out, const int c4, const int& t, const int& hf, const int& tid) {
    constexpr int CPP = HC / 8;
#pragma unroll
    for (int i = 0; i < TM * CPP / NTHR; ++i) {
        const int c = tid + NTHR * i, px = c / CPP, ch = c % CPP;
        *reinterpret_cast<uint4*>(out + ((long long)t * TM + px) * c4 + hf * HC + ch * 8) = *reinterpret_cast<const uint4*>(s_t + px * TPITCH + ch * 16);
        if (i & 1) __builtin_amdgcn_sched_barrier(0);
    }
}

// XCD-aware tile order of a persistent grid: workgroup bid of nblk walks tiles t0, t0 + tstep, ... < tend.  Workgroups are dealt round-robin
// to the 8 XCDs, so with nblk and ntiles multiples of 8 the workgroups of one XCD walk one contiguous eighth of the tiles (whole images: halo
// rows hit the same L2); otherwise the plain stride.
__host__ __device__ inline void xcd_tile_range(int nblk, unsigned bid, int ntiles, int& t0, int& tstep, int& tend) {
    if ((nblk & 7) == 0 && ntiles % 8 == 0) {
        const int per = ntiles >> 3;
        t0 = (bid & 7) * per + (bid >> 3); tstep = nblk >> 3; tend = ((bid & 7) + 1) * per;
    } else { t0 = bid; tstep = nblk; tend = ntiles; }
}

}  // namespace chain
}  // namespace dir
