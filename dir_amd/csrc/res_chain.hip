// dir_residual_chain_forward: one hourglass Residual block (Cin = 512, mid = 128, Cout = 256, stride 1) in ONE kernel (16-bit storage)
//   models/backbone/hourglass.py:33-70   out = conv3(relu(bn3(conv2(relu(bn2(conv1(relu(bn1(x)))))))) + skip_layer(x)
// Unfused the block is three launches (dir_amd/engine/decoder.py::ResidualOp): c1 1x1 with the pre-activation, c2 3x3, and conv3 + skip_layer as one GEMM
// over two K ranges.  On a 32x32 map at B = 64 they move 235 MB -- x twice, y1 and y2 written and read back -- for 101 MB of x + out.  Here y1 and
// y2 never leave the CU.
//
// One persistent 8-wave workgroup per CU walks 8x16-pixel tiles of one image.  Every GEMM is D[channel][pixel] (weights = MFMA A operand, as in
// bneck.hip): a lane holds 4 consecutive channels of a pixel, which is what the hand-over through LDS wants.  Per tile:
//   A. c1 on the 10x18 halo patch (192 pixel columns, 180 real): x arrives in 64-channel chunks global -> registers (two chunks ahead) -> LDS
//      (double buffer) with bn1 + ReLU applied on the way (convk::prologue's arithmetic), bn2 + ReLU -> y1 patch in LDS, rounded to the storage kind.  Patch
//      positions outside the image hold ZERO (conv2 pads y1, not x).  The halo is recomputed by the neighbouring tiles: 1.4x of c1's work, and
//      no hand-off between workgroups.
//   B. c2 3x3 from the y1 patch, bn3 + ReLU -> y2 tile in LDS, same rounding point.
//   C. conv3 + skip_layer: K range 1 = y2 (LDS), K range 2 = x of the tile's own 128 pixels, read again (L2 / Infinity Cache: this workgroup
//      has just read them) in 64-channel chunks through the same double buffer; + bias sum -> out through an LDS stage, 16-byte coalesced stores
//      into the destination's channel slice.
// The weights (w1 128 KB, w2 288 KB, w3 | skip 320 KB) do not fit a CU: every wave streams its MFMA A fragments from L2 in the order it consumes
// them -- ONE stream of 36 steps per tile (8 + 18 + 10; a step = 4 k-steps of 16 channels = 4 fragments of 1 KB) through a register ring two steps
// ahead, running across the phase boundaries and into the next tile.  The host packs them once (dir_amd/packing.py::pack_as_weights with A = 1).
// Every global load is unconditional (clamped address): a load inside a branch makes hipcc wait for everything at the join (stream.hip).
//
// fp32 accumulation in the K order and k-slot assignment of conv.hip (stream.hip's header): 64-channel slab outer, taps inner; MFMA ks of a slab
// multiplies channels 8 ks .. + 8 in lanes 0-31 and 32 + 8 ks .. + 8 in lanes 32-63; epilogues fmaf(acc, scale, shift) -> round -> ReLU.  The sums
// are the same fp32 chains as the three launches', the output is bit-identical.
#include "chain_common.h"

namespace dir {
namespace {

using namespace chain;
using convk::f16s_t;

constexpr int RC_CIN = 512, RC_MID = 128, RC_COUT = 256;
constexpr int TH = 8, TW = 16, NPX = TH * TW;              // tile: 128 pixels, P = row * 16 + col
constexpr int PH = TH + 2, PWD = TW + 2, NPP = PH * PWD;   // halo patch 10 x 18 = 180 positions, pp = pr * 18 + pc
constexpr int NPPAD = 192;                                 // ... as 6 MFMA column blocks
constexpr int NTHR = 512;
constexpr int XPITCH = 144;                                // bytes per pixel of an x chunk: 64 channels + 16 (conflict-free 16-lane reads)
constexpr int YPITCH = 272;                                // bytes per y1 / y2 pixel: 128 channels + 16
constexpr int Y1ROW = 5120;                                // bytes per y1 patch row: 18 x 272 rounded up to a multiple of 256, so that the two
                                                           // image rows a 32-pixel block spans stay 16 positions apart in bank groups
constexpr int OPITCH = 528;                                // bytes per staged output pixel: 256 channels + 16
constexpr int XBUF = NPPAD * XPITCH;                       // 27 648
constexpr int Y1BYTES = PH * Y1ROW;                        // 51 200
constexpr int Y2BYTES = NPX * YPITCH;                      // 34 816
static_assert(NPX * OPITCH <= Y1BYTES + Y2BYTES, "the output stage lies over y1 | y2");
constexpr int NSTEP = 36, STEP_B = 8, STEP_C = 26;         // weight steps per tile: c1 8, c2 18 (slab x tap), dual 10
constexpr int FRAG = 4 * 64;                               // uint4 per step and wave

struct ResArgs {
    const void* x; void* out;
    const uint4* w1; const uint4* w2; const uint4* w3;
    const float* pre_sc; const float* pre_sh; const float* sc1; const float* sh1; const float* sc2; const float* sh2; const float* sh3;
    int B, H, W, in_cs, in_co, out_cs, out_co, tiles_x, tiles_y, ntiles;
};

template <typename H>
__global__ __launch_bounds__(NTHR, 1) void res_chain_kernel(ResArgs a) {
    convk::half_kernel_init<H>();
    __shared__ __attribute__((aligned(16))) char s_x[2][XBUF];
    __shared__ __attribute__((aligned(16))) char s_y[Y1BYTES + Y2BYTES];          // y1 patch | y2 tile; the output stage at the end of a tile
    __shared__ __attribute__((aligned(16))) float s_pre[2 * RC_CIN];               // bn1 scale | shift
    __shared__ __attribute__((aligned(16))) float s_ss[4 * RC_MID + RC_COUT];      // sc1 sh1 | sc2 sh2 | sh3
    char* const s_y1 = s_y;
    char* const s_y2 = s_y + Y1BYTES;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l32 = lane & 31, h = lane >> 5;
    const unsigned short* __restrict__ xg = (const unsigned short*)a.x;
    unsigned short* __restrict__ og = (unsigned short*)a.out;

    for (int i = tid; i < RC_CIN; i += NTHR) { s_pre[i] = a.pre_sc[i]; s_pre[RC_CIN + i] = a.pre_sh[i]; }
    if (tid < RC_MID) {
        s_ss[tid] = a.sc1[tid]; s_ss[RC_MID + tid] = a.sh1[tid];
        s_ss[2 * RC_MID + tid] = a.sc2[tid]; s_ss[3 * RC_MID + tid] = a.sh2[tid];
    }
    if (tid < RC_COUT) s_ss[4 * RC_MID + tid] = a.sh3[tid];

    // ---- roles.  A and B: wave = (32-channel block cb of 4) x (pixel-block group pg of 2); C: wave = 32-channel block of 8, all 4 pixel blocks
    const int cb = wave & 3, pg = wave >> 2;
    // (buffer loads: a per-wave byte offset in one VGPR per matrix, the step as the scalar offset.  With flat pointers the compiler kept one hoisted
    //  64-bit address per fragment in VGPRs, which spilled)
    const __amdgpu_buffer_rsrc_t r1 = __builtin_amdgcn_make_buffer_rsrc((void*)a.w1, 0, RC_MID * RC_CIN * 2, 0x00020000);
    const __amdgpu_buffer_rsrc_t r2 = __builtin_amdgcn_make_buffer_rsrc((void*)a.w2, 0, RC_MID * 9 * RC_MID * 2, 0x00020000);
    const __amdgpu_buffer_rsrc_t r3 = __builtin_amdgcn_make_buffer_rsrc((void*)a.w3, 0, RC_COUT * (RC_MID + RC_CIN) * 2, 0x00020000);
    const int vA = (cb * 8 * FRAG + lane) * 16, vB = (cb * 18 * FRAG + lane) * 16, vC = (wave * 10 * FRAG + lane) * 16;
    convk::u32x4 wr[3][4];                                                        // ring: step s sits in wr[s % 3]
    auto wload = [&](auto S) {                                                    // step S of the tile's stream (S >= 36: the next tile's)
        constexpr int s = decltype(S)::value % NSTEP;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            if constexpr (s < STEP_B) wr[decltype(S)::value % 3][ks] = __builtin_bit_cast(convk::u32x4, __builtin_amdgcn_raw_buffer_load_b128(r1, vA, (s * FRAG + ks * 64) * 16, 0));
            else if constexpr (s < STEP_C) wr[decltype(S)::value % 3][ks] = __builtin_bit_cast(convk::u32x4, __builtin_amdgcn_raw_buffer_load_b128(r2, vB, ((s - STEP_B) * FRAG + ks * 64) * 16, 0));
            else wr[decltype(S)::value % 3][ks] = __builtin_bit_cast(convk::u32x4, __builtin_amdgcn_raw_buffer_load_b128(r3, vC, ((s - STEP_C) * FRAG + ks * 64) * 16, 0));
        }
    };

    int t0, tstep, tend;
    xcd_tile_range(gridDim.x, blockIdx.x, a.ntiles, t0, tstep, tend);

    wload(IC<0>{});
    wload(IC<1>{});
    __syncthreads();                                                              // s_pre, s_ss

    for (int t = t0; t < tend; t += tstep) {
        const int tx = t % a.tiles_x, r_ = t / a.tiles_x, b = r_ / a.tiles_y, y0 = (r_ - b * a.tiles_y) * TH, x0 = tx * TW;

        // ---- x addressing.  Phase A: piece e = tid + 512 i (i < 3) = patch position e >> 3 (clamped into the image; positions >= 180 are
        //      padding columns nobody reads back), 16-byte channel piece e & 7.  Phase C: piece e (i < 2) = tile pixel e >> 3.
        const int cc = tid & 7;
        unsigned offA[3], offC[2];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int pp = min((tid + NTHR * i) >> 3, NPP - 1), pr = pp / PWD, pc = pp - pr * PWD;
            const int iy = min(max(y0 - 1 + pr, 0), a.H - 1), ix = min(max(x0 - 1 + pc, 0), a.W - 1);
            offA[i] = (unsigned)(((b * a.H + iy) * a.W + ix) * a.in_cs + a.in_co + cc * 8);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int P = (tid + NTHR * i) >> 3;
            offC[i] = (unsigned)(((b * a.H + y0 + (P >> 4)) * a.W + x0 + (P & 15)) * a.in_cs + a.in_co + cc * 8);
        }
        uint4 xa[2][3];
        auto loadA = [&](auto Set, int c) {
#pragma unroll
            for (int i = 0; i < 3; ++i) xa[decltype(Set)::value][i] = *reinterpret_cast<const uint4*>(xg + offA[i] + min(c, 7) * 64);
        };
        auto storeA = [&](auto Set, int c, int buf) {
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const int pp = (tid + NTHR * i) >> 3;
                // convk::prologue<H> (fma in fp32, ReLU, round) with the ReLU taken on the packed pairs after rounding: rounding is monotonic and keeps the
                // sign, so the bits are the same (conv_common.h: OutVecHalf::store_act), for half the maximum instructions -- this phase is VALU-bound
                const uint4 v = xa[decltype(Set)::value][i];
                const uint32_t u[4] = {v.x, v.y, v.z, v.w};
                const float4 s0 = *reinterpret_cast<const float4*>(s_pre + c * 64 + cc * 8), s1 = *reinterpret_cast<const float4*>(s_pre + c * 64 + cc * 8 + 4);
                const float4 b0 = *reinterpret_cast<const float4*>(s_pre + RC_CIN + c * 64 + cc * 8), b1 = *reinterpret_cast<const float4*>(s_pre + RC_CIN + c * 64 + cc * 8 + 4);
                const float ps[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w}, pb[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
                uint32_t o[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float lo, hi;
                    convk::unpack2<H>(u[e], lo, hi);
                    o[e] = Half<H>::pack2_relu(fmaf(lo, ps[2 * e], pb[2 * e]), fmaf(hi, ps[2 * e + 1], pb[2 * e + 1]));
                }
                *reinterpret_cast<uint4*>(s_x[buf] + pp * XPITCH + cc * 16) = make_uint4(o[0], o[1], o[2], o[3]);
            }
        };
        auto loadC = [&](auto Set, int c) {
#pragma unroll
            for (int i = 0; i < 2; ++i) xa[decltype(Set)::value][i] = *reinterpret_cast<const uint4*>(xg + offC[i] + min(c, 7) * 64);
        };
        auto storeC = [&](auto Set, int buf) {
#pragma unroll
            for (int i = 0; i < 2; ++i) *reinterpret_cast<uint4*>(s_x[buf] + ((tid + NTHR * i) >> 3) * XPITCH + cc * 16) = xa[decltype(Set)::value][i];
        };
        using I0 = IC<0>;
        using I1 = IC<1>;

        // ================================================================ A. c1 on the patch: 32 channels x 96 patch positions per wave
        loadA(I0{}, 0);
        loadA(I1{}, 1);
        storeA(I0{}, 0, 0);
        loadA(I0{}, 2);
        __syncthreads();                                                          // chunk 0 visible (and the previous tile's stage is drained)
        {
            f32x16 acc[3];
#pragma unroll
            for (int j = 0; j < 3; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
            const char* bA = s_x[0] + (96 * pg + l32) * XPITCH + 64 * h;
            [&]<int... Cs>(std::integer_sequence<int, Cs...>) {
                (([&] {
                     constexpr int c = Cs;
                     __builtin_amdgcn_sched_barrier(0);                          // a step's reads stay inside the step (unrolled, they were hoisted until the registers ran out)
                     wload(IC<c + 2>{});
                     const char* bp = bA + (c & 1) * XBUF;
                     uint4 bv[2][3];                                              // the pixels' channels (MFMA B operands), read a k-step ahead
#pragma unroll
                     for (int j = 0; j < 3; ++j) bv[0][j] = *reinterpret_cast<const uint4*>(bp + 32 * j * XPITCH);
#pragma unroll
                     for (int ks = 0; ks < 4; ++ks) {
                         if (ks + 1 < 4) {
#pragma unroll
                             for (int j = 0; j < 3; ++j) bv[(ks + 1) & 1][j] = *reinterpret_cast<const uint4*>(bp + 32 * j * XPITCH + 16 * (ks + 1));
                         }
                         __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                         for (int j = 0; j < 3; ++j) acc[j] = Half<H>::mfma32(wr[c % 3][ks], bv[ks & 1][j], acc[j]);
                     }
                     if constexpr (c + 1 < 8) {                                   // chunk c + 1 -> the other buffer (free since the last barrier); c + 3 on its way
                         storeA(IC<(c + 1) & 1>{}, c + 1, (c + 1) & 1);
                         if constexpr (c + 3 < 8) loadA(IC<(c + 1) & 1>{}, c + 3);
                     } else {                                                     // the tile's own pixels for phase C, chunks 0 and 1: in flight during phase B
                         loadC(I0{}, 0);
                         loadC(I1{}, 1);
                     }
                     __syncthreads();
                 }()),
                 ...);
            }(std::make_integer_sequence<int, 8>{});
            // bn2 + ReLU -> y1 patch; rows (channels) of the 32x32 tile held by this lane: 8 q + 4 h + {0..3}
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const int pp = 96 * pg + 32 * j + l32, pr = pp / PWD, pc = pp - pr * PWD;
                const int iy = y0 - 1 + pr, ix = x0 - 1 + pc;
                const bool in = iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
                if (pp < NPP) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int c0 = 32 * cb + 8 * q + 4 * h;
                        const float4 sc = *reinterpret_cast<const float4*>(s_ss + c0);
                        const float4 sh = *reinterpret_cast<const float4*>(s_ss + RC_MID + c0);
                        uint2 o = bn_relu4<H>(acc[j], q, sc, sh);
                        if (!in) o = make_uint2(0u, 0u);
                        *reinterpret_cast<uint2*>(s_y1 + pr * Y1ROW + pc * YPITCH + c0 * 2) = o;
                    }
                }
            }
        }
        __syncthreads();                                                          // y1 patch complete; both x buffers free

        // ================================================================ B. c2 3x3: 32 channels x 64 pixels per wave, K = 2 slabs x 9 taps x 64
        {
            f32x16 acc[2];
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
            // pixel P = 64 pg + 32 j + l32: tile row 4 pg + 2 j + (l32 >> 4), column l32 & 15
            const char* bB = s_y1 + (4 * pg + (l32 >> 4)) * Y1ROW + (l32 & 15) * YPITCH + 64 * h;
            uint4 bv[2][2];                                                       // MFMA B operands, read a k-step ahead (across the steps: no barrier in this phase)
            auto bread = [&](auto I) {                                            // k-step I = 4 step + ks of the phase
                constexpr int i = decltype(I)::value, s = i >> 2, ks = i & 3, slab = s / 9, tap = s % 9, ky = tap / 3, kx = tap % 3;
#pragma unroll
                for (int j = 0; j < 2; ++j) bv[i & 1][j] = *reinterpret_cast<const uint4*>(bB + (ky + 2 * j) * Y1ROW + kx * YPITCH + slab * 128 + 16 * ks);
            };
            bread(IC<0>{});
            [&]<int... Ss>(std::integer_sequence<int, Ss...>) {
                (([&] {
                     constexpr int s = Ss;                                        // step = slab * 9 + tap: 64-channel slab outer, taps inner
                     __builtin_amdgcn_sched_barrier(0);
                     wload(IC<STEP_B + s + 2>{});
                     [&]<int... Ks>(std::integer_sequence<int, Ks...>) {
                         (([&] {
                              constexpr int i = 4 * s + Ks;
                              if constexpr (i + 1 < 72) bread(IC<i + 1>{});
                              __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                              for (int j = 0; j < 2; ++j) acc[j] = Half<H>::mfma32(wr[(STEP_B + s) % 3][Ks], bv[i & 1][j], acc[j]);
                          }()),
                          ...);
                     }(std::make_integer_sequence<int, 4>{});
                 }()),
                 ...);
            }(std::make_integer_sequence<int, 18>{});
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int c0 = 32 * cb + 8 * q + 4 * h;
                    const float4 sc = *reinterpret_cast<const float4*>(s_ss + 2 * RC_MID + c0);
                    const float4 sh = *reinterpret_cast<const float4*>(s_ss + 3 * RC_MID + c0);
                    *reinterpret_cast<uint2*>(s_y2 + (64 * pg + 32 * j + l32) * YPITCH + c0 * 2) = bn_relu4<H>(acc[j], q, sc, sh);
                }
        }
        storeC(I0{}, 0);                                                          // x chunk 0 of the tile's pixels (requested at the end of phase A)
        loadC(I0{}, 2);
        __syncthreads();                                                          // y2 and x chunk 0 visible

        // ================================================================ C. conv3 + skip_layer: 32 channels x 128 pixels per wave, K = 128 (y2) + 512 (x)
        {
            f32x16 acc[4];
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
            [&]<int... Ss>(std::integer_sequence<int, Ss...>) {
                (([&] {
                     constexpr int s = Ss;                                        // chunk of the dual GEMM: 0, 1 = y2; 2 .. 9 = x chunk s - 2
                     __builtin_amdgcn_sched_barrier(0);
                     wload(IC<STEP_C + s + 2>{});
                     const char* bp = s < 2 ? s_y2 + l32 * YPITCH + s * 128 + 64 * h : s_x[s & 1] + l32 * XPITCH + 64 * h;
                     constexpr int pitch = s < 2 ? YPITCH : XPITCH;
                     uint4 bv[2][4];
#pragma unroll
                     for (int j = 0; j < 4; ++j) bv[0][j] = *reinterpret_cast<const uint4*>(bp + 32 * j * pitch);
#pragma unroll
                     for (int ks = 0; ks < 4; ++ks) {
                         if (ks + 1 < 4) {
#pragma unroll
                             for (int j = 0; j < 4; ++j) bv[(ks + 1) & 1][j] = *reinterpret_cast<const uint4*>(bp + 32 * j * pitch + 16 * (ks + 1));
                         }
                         __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                         for (int j = 0; j < 4; ++j) acc[j] = Half<H>::mfma32(wr[(STEP_C + s) % 3][ks], bv[ks & 1][j], acc[j]);
                     }
                     if constexpr (s >= 2 && s < 9) {                             // x chunk s - 1 -> buffer (s + 1) & 1 (free since the last barrier); s + 1 on its way
                         storeC(IC<(s + 1) & 1>{}, (s + 1) & 1);
                         if constexpr (s + 1 < 8) loadC(IC<(s + 1) & 1>{}, s + 1);
                         __syncthreads();
                     }
                 }()),
                 ...);
            }(std::make_integer_sequence<int, 10>{});
            __syncthreads();                                                      // every wave is done with y2 and the x buffers: the stage may overwrite y1 | y2
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int c0 = 32 * wave + 8 * q + 4 * h;
                    const float4 sh = *reinterpret_cast<const float4*>(s_ss + 4 * RC_MID + c0);
                    uint2 o;
                    o.x = Half<H>::pack2(fmaf(acc[j][4 * q], 1.f, sh.x), fmaf(acc[j][4 * q + 1], 1.f, sh.y));
                    o.y = Half<H>::pack2(fmaf(acc[j][4 * q + 2], 1.f, sh.z), fmaf(acc[j][4 * q + 3], 1.f, sh.w));
                    *reinterpret_cast<uint2*>(s_y + (32 * j + l32) * OPITCH + c0 * 2) = o;
                }
        }
        __syncthreads();
        // out: piece e = tid + 512 i = pixel e >> 5, 16-byte channel piece e & 31 -- two whole 512-byte pixels per wave instruction
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int e = tid + NTHR * i, P = e >> 5, oc = e & 31;
            *reinterpret_cast<uint4*>(og + ((long long)(b * a.H + y0 + (P >> 4)) * a.W + x0 + (P & 15)) * a.out_cs + a.out_co + oc * 8) =
                *reinterpret_cast<const uint4*>(s_y + P * OPITCH + oc * 16);
        }
        // (the next tile writes s_x only before its first barrier, and y1 only after eight more: the stage is read out by then)
    }
}

}  // namespace
}  // namespace dir

extern "C" int dir_residual_chain_supported(int dtype, int Cin, int Cmid, int Cout, int B, int H, int W, int in_cstride, int in_coff, int out_cstride, int out_coff) {
    using namespace dir;
    if (dtype != DIR_DT_BF16 && dtype != DIR_DT_F16) return 0;
    if (Cin != RC_CIN || Cmid != RC_MID || Cout != RC_COUT || B <= 0) return 0;
    if (!((H == 32 && W == 32) || (H == 16 && W == 16))) return 0;
    if (in_cstride < in_coff + Cin || in_coff < 0 || in_cstride % 8 || in_coff % 8) return 0;
    if (out_cstride < out_coff + Cout || out_coff < 0 || out_cstride % 8 || out_coff % 8) return 0;
    if ((long long)B * H * W * in_cstride >= (1ll << 31) || (long long)B * H * W * out_cstride >= (1ll << 31)) return 0;
    return 1;
}

extern "C" int dir_residual_chain_forward(const dir_res_chain_params* p, const void* x, void* out, int B, int H, int W, int in_cstride, int in_coff,
                                          int out_cstride, int out_coff, void* stream) {
    using namespace dir;
    DIR_REQUIRE(p && x && out, "dir_residual_chain_forward: null pointer");
    DIR_REQUIRE(p->w1 && p->w2 && p->w3 && p->pre_scale && p->pre_shift && p->scale1 && p->shift1 && p->scale2 && p->shift2 && p->shift3,
                "dir_residual_chain_forward: missing parameters");
    DIR_REQUIRE(dir_residual_chain_supported(p->dtype, p->Cin, p->Cmid, p->Cout, B, H, W, in_cstride, in_coff, out_cstride, out_coff),
                "dir_residual_chain_forward: unsupported (bf16 / f16 storage, 512 -> 128 -> 256, 32x32 or 16x16 maps, channel strides and offsets "
                "multiples of 8, tensors below 2^31 elements)");
    ResArgs a;
    a.x = x; a.out = out;
    a.w1 = (const uint4*)p->w1; a.w2 = (const uint4*)p->w2; a.w3 = (const uint4*)p->w3;
    a.pre_sc = p->pre_scale; a.pre_sh = p->pre_shift; a.sc1 = p->scale1; a.sh1 = p->shift1; a.sc2 = p->scale2; a.sh2 = p->shift2; a.sh3 = p->shift3;
    a.B = B; a.H = H; a.W = W; a.in_cs = in_cstride; a.in_co = in_coff; a.out_cs = out_cstride; a.out_co = out_coff;
    a.tiles_x = W / TW; a.tiles_y = H / TH; a.ntiles = B * a.tiles_x * a.tiles_y;
    const int grid = persistent_grid(a.ntiles);
    hipStream_t s = (hipStream_t)stream;
    if (p->dtype == DIR_DT_F16) DIR_LAUNCH((res_chain_kernel<f16s_t>), dim3(grid), dim3(NTHR), 0, s, a);
    else DIR_LAUNCH((res_chain_kernel<bf16_t>), dim3(grid), dim3(NTHR), 0, s, a);
    return check_launch("dir_residual_chain_forward");
}
