// dir_bottleneck_block_forward: one ResNet layer3 identity bottleneck from conv2 on -- and the 1x1 head of the next one -- in ONE kernel
// (16-bit storage; planes P = 256, block width C4 = 1024, 16-wide maps, stride 1):
//   models/backbone/resnet.py:126-130   block i  : conv2 3x3 (P -> P) -> bn2 -> ReLU                                  -> y2   (stays on the CU)
//   models/backbone/resnet.py:132-140   block i  : conv3 1x1 (P -> 4P) -> bn3 -> += identity -> ReLU                   -> out  (HBM)
//   models/backbone/resnet.py:122-124   block i+1: conv1 1x1 (4P -> N2) -> bn1 -> ReLU                                 -> y1n  (HBM; N2 = 256, or 0: none)
// Unfused this is conv_as.hip's 3x3 followed by tail.hip (or, for the layer's last block, by conv3 as a convolution with a residual): two launches,
// each with its own ramp, first-load latency and drain, and y2 written to memory and read back.  The launch boundary stays at y1, where the
// previous launch leaves it: the 3x3 reads its halo of y1 from memory as conv_as does -- no halo recompute, no hand-off between workgroups.
//
// One persistent 8-wave workgroup per CU walks 64-pixel tiles: four whole rows of one 16-wide image (conv_as's (A, PB) = (2, 2) ownership, and a
// legal tail.hip tile: 64 consecutive NHW pixels).  Every GEMM is D[channel][pixel] (weights = MFMA A operand).  Per tile:
//   A. conv2: the 6 x 18 x 256 halo patch of y1 global -> registers -> LDS (zeros outside the image); wave w owns output channels [32 w, 32 w + 32)
//      x both 32-pixel blocks; bn2 + ReLU, rounded to the storage kind (the rounding point of the stored y2) -> y2 [64][256] in LDS.
//   B. conv3, per 512-channel half: y2 (LDS) x this wave's 64 channels, bn3 + identity + ReLU -> T [64][512] in LDS (over the dead patch), rounded
//      as tail.hip does; the identity rows sit in registers a unit ahead; T -> out with 16-byte coalesced stores.
//   C. next conv1 (N2 = 256): T x this wave's 32 channels, accumulated over the halves in registers; bn1 + ReLU -> y1n.
// The weights (w2 1.1 MB, w3 0.5 MB, w1n 0.5 MB) do not fit a CU: every wave streams its MFMA A fragments from L2 through a register ring in the
// order it consumes them -- ONE stream per wave (144 conv2 fragments, then per half 32 conv3 and 32 conv1 fragments), running across the phases
// and into the next tile; the host packs it (dir_amd/packing.py::pack_l3_stream).
//
// fp32 chains: conv2 has conv.hip's K order and k-slots (64-channel slab outer, taps inner; MFMA ks of a slab multiplies channels 8 ks .. + 8 in
// lanes 0-31 and 32 + 8 ks .. + 8 in lanes 32-63).  conv3 and conv1 have tail.hip's where the next conv1 is fused (k-step ks = channels
// 16 ks + 8 h .. + 8); with N2 = 0 conv3 has conv.hip's, because the launch it replaces is then a convolution.  Either way the output is
// bit-identical to the launches replaced.
// No flags, no counters, no dependence between workgroups.
#include "chain_common.h"

namespace dir {
namespace {

using namespace chain;
using convk::f16s_t;

constexpr int P = 256, C4 = 1024;      // planes, block width
constexpr int TM = 64;                 // pixels per tile: 4 rows x 16 columns
constexpr int HC = 512;                // channels per half of the block output
constexpr int NTHR = 512;
constexpr int TPITCH = HC * 2 + 16;    // bytes per T pixel
constexpr int YPITCH = P * 2 + 16;     // bytes per y1 patch position / y2 pixel: the 16-byte skew spreads 16 consecutive positions over the bank groups
constexpr int PROW = 9728;             // bytes per patch row: 18 x 528 rounded up to a multiple of 256, so that the two image rows of a 32-pixel
                                       // block fall on the same bank groups 16 lanes apart (res_chain.hip)
constexpr int PATCH = 6 * PROW;        // 58 368
constexpr int R0 = TM * TPITCH > PATCH ? TM * TPITCH : PATCH;      // the patch, then T over it: 66 560
constexpr int GRP = 8;                 // weight fragments per ring group (1 KB each per wave)
constexpr int NAF = 144;               // conv2 fragments per tile and wave: 4 slabs x 9 taps x 4 k-steps
constexpr int NBF = 32;                // conv3 fragments per half: 2 channel blocks x 16 k-steps

struct L3Args {
    const bf16_t* y1; const bf16_t* res; bf16_t* out; bf16_t* y1n;
    const uint4* wstream;              // [8 waves][NAF + 2 (NBF + NCF) fragments][64 lanes] x 16 bytes
    const float* sc2; const float* sh2; const float* sc3; const float* sh3; const float* sc1n; const float* sh1n;
    int H, tiles_per_img, ntiles;
};

// N2: output channels of the fused next conv1 (256), or 0: none (the layer's last block)
template <int N2, typename H>
__global__ __launch_bounds__(NTHR, 1) void l3_chain_kernel(L3Args a) {
    convk::half_kernel_init<H>();
    constexpr bool NEXT = N2 != 0;
    constexpr int NCF = NEXT ? HC / 16 : 0;             // conv1 fragments per half
    constexpr int NUF = NBF + NCF;                      // fragments per unit (tile, half)
    constexpr int NF = NAF + 2 * NUF;                   // ... per tile
    constexpr int NGA = NAF / GRP, NGU = NUF / GRP;
    static_assert(NAF % (2 * GRP) == 0 && NUF % (2 * GRP) == 0 && (N2 == 0 || N2 == 256), "l3_chain_kernel: the ring slot of a group must be compile-time");
    __shared__ __attribute__((aligned(16))) char s_r0[R0];                     // the y1 patch (phase A), then T
    __shared__ __attribute__((aligned(16))) char s_y2[TM * YPITCH];
    __shared__ __attribute__((aligned(16))) float s_ss[2 * P + 2 * C4 + 2 * N2 + 4];      // sc2 | sh2 | sc3 | sh3 | sc1n | sh1n
    char* const s_t = s_r0;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l32 = lane & 31, h = lane >> 5;

    int t0, tstep, tend;
    xcd_tile_range(gridDim.x, blockIdx.x, a.ntiles, t0, tstep, tend);
    if (t0 >= tend) return;

    // ---- weight stream of this wave: fragment f of a tile at wstream[(wave * NF + f) * 64 + lane]
    //      (buffer loads, as res_chain.hip: one byte offset per wave in a VGPR, the fragment as the scalar offset; with flat pointers the
    //      compiler keeps one hoisted 64-bit address per fragment in VGPRs, which spill)
    const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc((void*)a.wstream, 0, 8 * NF * 1024, 0x00020000);
    const int wv = (wave * NF * 64 + lane) * 16;
    convk::u32x4 ring[2][GRP];
    auto ring_load = [&](auto Slot, auto F0) {
        constexpr int slot = decltype(Slot)::value, f0 = decltype(F0)::value;
#pragma unroll
        for (int i = 0; i < GRP; ++i) ring[slot][i] = __builtin_bit_cast(convk::u32x4, __builtin_amdgcn_raw_buffer_load_b128(wrs, wv, (f0 + i) * 1024, 0));
    };
    ring_load(IC<0>{}, IC<0>{});

    for (int i = tid; i < P; i += NTHR) { s_ss[i] = a.sc2[i]; s_ss[P + i] = a.sh2[i]; }
    for (int i = tid; i < C4; i += NTHR) { s_ss[2 * P + i] = a.sc3[i]; s_ss[2 * P + C4 + i] = a.sh3[i]; }
    if constexpr (NEXT) {
        for (int i = tid; i < N2; i += NTHR) { s_ss[2 * P + 2 * C4 + i] = a.sc1n[i]; s_ss[2 * P + 2 * C4 + N2 + i] = a.sh1n[i]; }
    }
    const float* const s_sc3 = s_ss + 2 * P;
    const float* const s_sh3 = s_ss + 2 * P + C4;

    // ---- identity rows of a unit as 16-byte chunks, turned into the epilogue-B layout where they are used (chain_common.h: res16_fetch / res16_take)
    uint4 xr[2][2][2];
    auto res_fetch = [&](int tile, int half) {
#pragma unroll
        for (int pb = 0; pb < 2; ++pb) {
            const bf16_t* rp = a.res + ((long long)tile * TM + 32 * pb + l32) * C4 + half * HC + 64 * wave + 8 * h;
#pragma unroll
            for (int cb = 0; cb < 2; ++cb) res16_fetch(rp + 32 * cb, xr[cb][pb]);
        }
    };

    f32x16 accc[2];                                      // next conv1: [pixel block], accumulated over the halves
    uint4 bop[2][2];                                     // activation (MFMA B) operands of a fragment step, read one step ahead
    auto act_read = [&](auto F, auto Set) {
        constexpr int f = decltype(F)::value, set = decltype(Set)::value;
        if constexpr (f < NBF) {
            constexpr int ks = f % 16;
            // fused next conv1: tail.hip's k-slots (channels 16 ks + 8 h ..); else conv.hip's (slab ks / 4: channels 64 slab + 32 h + 8 (ks % 4) ..)
            constexpr int koff = NEXT ? 32 * ks : 128 * (ks >> 2) + 16 * (ks & 3);
#pragma unroll
            for (int pb = 0; pb < 2; ++pb)
                bop[set][pb] = *reinterpret_cast<const uint4*>(s_y2 + (32 * pb + l32) * YPITCH + koff + (NEXT ? 16 : 64) * h);
        } else {                                         // T[pixel 32 pb + l32][16 fc + 8 h ..]
            constexpr int fc = f - NBF;
#pragma unroll
            for (int pb = 0; pb < 2; ++pb) bop[set][pb] = *reinterpret_cast<const uint4*>(s_t + (32 * pb + l32) * TPITCH + 32 * fc + 16 * h);
        }
    };

    for (int t = t0; t < tend; t += tstep) {
        const int img = t / a.tiles_per_img, trow = (t - img * a.tiles_per_img) * 4;

        // ---- the y1 patch: rows trow - 1 .. trow + 4, all 16 columns, 256 channels: piece (row i, pixel tid >> 5, 16-byte chunk tid & 31), the
        //      address clamped into the image and the value zero-selected (conv2 pads y1 with zeros).  Columns 0 and 17 of the patch are always
        //      outside a 16-wide image.  Region 0 is free: the previous tile's closing barrier.
        {
            const int px = tid >> 5, ch = tid & 31;
            uint4 pv[6];
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                const int iy = trow - 1 + i, iyc = min(max(iy, 0), a.H - 1);
                pv[i] = *reinterpret_cast<const uint4*>(a.y1 + (((long long)img * a.H + iyc) * 16 + px) * P + ch * 8);
                if (iy != iyc) pv[i] = make_uint4(0u, 0u, 0u, 0u);
            }
            res_fetch(t, 0);
#pragma unroll
            for (int i = 0; i < 6; ++i) *reinterpret_cast<uint4*>(s_r0 + i * PROW + (px + 1) * YPITCH + ch * 16) = pv[i];
            if (tid < 384) *reinterpret_cast<uint4*>(s_r0 + (tid >> 6) * PROW + ((tid >> 5) & 1) * 17 * YPITCH + ch * 16) = make_uint4(0u, 0u, 0u, 0u);
        }
        __syncthreads();                                 // the patch (and, first tile, the BatchNorm vectors)

        // ================================================================ A. conv2 3x3: 32 channels x 64 pixels per wave, K = 4 slabs x 9 taps x 64
        {
            f32x16 acc[2];
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
            // pixel 32 j + l32: tile row 2 j + (l32 >> 4), column l32 & 15; patch row = tile row + ky, patch column = column + kx
            const char* bB = s_r0 + (l32 >> 4) * PROW + (l32 & 15) * YPITCH + 64 * h;
            auto bread = [&](auto I) {                   // fragment I = 4 step + ks; step = slab * 9 + tap: 64-channel slab outer, taps inner
                constexpr int i = decltype(I)::value, s = i >> 2, ks = i & 3, slab = s / 9, tap = s % 9, ky = tap / 3, kx = tap % 3;
#pragma unroll
                for (int j = 0; j < 2; ++j) bop[i & 1][j] = *reinterpret_cast<const uint4*>(bB + (ky + 2 * j) * PROW + kx * YPITCH + slab * 128 + 16 * ks);
            };
            bread(IC<0>{});
            [&]<int... G>(std::integer_sequence<int, G...>) {
                (([&] {
                     constexpr int grp = G, slot = G & 1;
                     __builtin_amdgcn_sched_barrier(0);
                     ring_load(IC<slot ^ 1>{}, IC<(G + 1) * GRP>{});           // the next group; after the last one: group 0 of the first unit
                     [&]<int... I>(std::integer_sequence<int, I...>) {
                         (([&] {
                              constexpr int i = grp * GRP + I;
                              if constexpr (i + 1 < NAF) bread(IC<i + 1>{});
                              __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                              for (int j = 0; j < 2; ++j) acc[j] = Half<H>::mfma32(ring[slot][I], bop[i & 1][j], acc[j]);
                          }()),
                          ...);
                     }(std::make_integer_sequence<int, GRP>{});
                 }()),
                 ...);
            }(std::make_integer_sequence<int, NGA>{});
            // bn2 + ReLU -> y2, rounded to the storage kind; rows (channels) of the 32x32 tile held by this lane: 8 q + 4 h + {0 .. 3}
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int c0 = 32 * wave + 8 * q + 4 * h;
                    const float4 sc = *reinterpret_cast<const float4*>(s_ss + c0);
                    const float4 sh = *reinterpret_cast<const float4*>(s_ss + P + c0);
                    *reinterpret_cast<uint2*>(s_y2 + (32 * j + l32) * YPITCH + c0 * 2) = bn_relu4<H>(acc[j], q, sc, sh);
                }
        }
        __syncthreads();                                 // y2 complete; every wave is done with the patch: T may take its place

        // ================================================================ B / C per 512-channel half (tail.hip's unit)
        auto unit = [&](auto HF) {
            constexpr int hf = decltype(HF)::value;
            constexpr bool last_half = hf == 1;
            constexpr int fbase = NAF + hf * NUF;
            f32x16 accb[2];                              // conv3: [pixel block] of the current channel block
            if constexpr (NEXT && hf == 0) {
#pragma unroll
                for (int pb = 0; pb < 2; ++pb)
#pragma unroll
                    for (int r = 0; r < 16; ++r) accc[pb][r] = 0.f;
            }
            act_read(IC<0>{}, IC<0>{});
            [&]<int... G>(std::integer_sequence<int, G...>) {
                (([&] {
                     constexpr int grp = G, slot = G & 1;
                     // the next group: of this unit, of the next unit, or group 0 of the next tile (the same stream again)
                     constexpr int fnext = G + 1 < NGU ? fbase + (G + 1) * GRP : last_half ? 0 : fbase + NUF;
                     ring_load(IC<slot ^ 1>{}, IC<fnext>{});
                     [&]<int... I>(std::integer_sequence<int, I...>) {
                         (([&] {
                              constexpr int f = grp * GRP + I, set = f & 1;
                              // operands of the next step (not across the phase boundary: T does not exist yet; not across the unit)
                              if constexpr (f + 1 < NUF && f + 1 != NBF) act_read(IC<f + 1>{}, IC<set ^ 1>{});
                              if constexpr (f < NBF) {
                                  // ---- B. conv3: fragment (channel block cb, k-step ks), channel-block-major
                                  constexpr int cb = f / 16, ks = f - cb * 16;
                                  if constexpr (ks == 0) {
#pragma unroll
                                      for (int pb = 0; pb < 2; ++pb)
#pragma unroll
                                          for (int r = 0; r < 16; ++r) accb[pb][r] = 0.f;
                                  }
#pragma unroll
                                  for (int pb = 0; pb < 2; ++pb) accb[pb] = Half<H>::mfma32(ring[slot][I], bop[set][pb], accb[pb]);
                                  if constexpr (ks == 15) {
                                      // ---- epilogue B of this channel block -> T: bn3 + identity + ReLU, rounded
                                      epilogue_b<H, TPITCH>(accb, xr[cb], s_sc3 + hf * HC, s_sh3 + hf * HC, s_t, 64 * wave + 32 * cb, l32, h);
                                  }
                                  if constexpr (f == NBF - 1) {
                                      __syncthreads();                               // T = this half of the block output
                                      if constexpr (NEXT) act_read(IC<NBF>{}, IC<set ^ 1>{});
                                      if constexpr (!last_half) res_fetch(t, hf + 1);     // into the registers just consumed
                                      store_t_to_out<NTHR, TM, HC, TPITCH>(s_t, a.out, C4, t, hf, tid);
                                  }
                              } else {
                                  // ---- C. next conv1 over this half's 512 input channels
#pragma unroll
                                  for (int pb = 0; pb < 2; ++pb) accc[pb] = Half<H>::mfma32(ring[slot][I], bop[set][pb], accc[pb]);
                              }
                              __builtin_amdgcn_sched_barrier(0);
                          }()),
                          ...);
                     }(std::make_integer_sequence<int, GRP>{});
                 }()),
                 ...);
            }(std::make_integer_sequence<int, NGU>{});
            if constexpr (NEXT && last_half) {
                // ---- epilogue C: bn1 + ReLU -> next y1, one 16-byte store per j (tail.hip's, kept in place in both: as one shared function it moved
                //      tail_chain_kernel<256, 256>'s register allocation)
                const float* const s_sc1 = s_ss + 2 * P + 2 * C4;
#pragma unroll
                for (int pb = 0; pb < 2; ++pb) {
                    uint2 o[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int c0 = 32 * wave + 8 * q + 4 * h;
                        const float4 sc = *reinterpret_cast<const float4*>(s_sc1 + c0);
                        const float4 sh = *reinterpret_cast<const float4*>(s_sc1 + N2 + c0);
                        o[q] = bn_relu4<H>(accc[pb], q, sc, sh);
                    }
                    store16_swapped(o, a.y1n + ((long long)t * TM + 32 * pb + l32) * N2 + 32 * wave + 8 * h);
                }
            }
            __syncthreads();                             // T (and after the last half y2) is free
        };
        unit(IC<0>{});
        unit(IC<1>{});
    }
}

}  // namespace
}  // namespace dir

extern "C" int dir_bottleneck_block_supported(int dtype, int planes, int n_next, int B, int H, int W) {
    if (dtype != DIR_DT_BF16 && dtype != DIR_DT_F16) return 0;
    if (planes != dir::P || !(n_next == 256 || n_next == 0)) return 0;
    if (B <= 0 || H <= 0 || W != 16 || H % 4) return 0;                      // a tile is four whole rows of a 16-wide image
    if ((long long)B * (H / 4) >= (1ll << 31)) return 0;                     // tiles (global offsets are 64-bit)
    return 1;
}

extern "C" int dir_bottleneck_block_forward(const dir_bneck_block_params* p, const void* y1, const void* residual, void* out, void* y1_next,
                                            int B, int H, int W, void* stream) {
    using namespace dir;
    DIR_REQUIRE(p && y1 && residual && out, "dir_bottleneck_block_forward: null pointer");
    DIR_REQUIRE(p->wstream && p->scale2 && p->shift2 && p->scale3 && p->shift3, "dir_bottleneck_block_forward: missing parameters");
    DIR_REQUIRE(dir_bottleneck_block_supported(p->dtype, p->planes, p->n_next, B, H, W),
                "dir_bottleneck_block_forward: unsupported (bf16 / f16 storage, planes 256, n_next 256 or 0, W = 16, H a multiple of 4)");
    DIR_REQUIRE(p->n_next == 0 || (y1_next && p->scale1n && p->shift1n), "dir_bottleneck_block_forward: null pointer (the fused next conv1 needs y1_next, scale1n and shift1n)");
    L3Args a;
    a.y1 = (const convk::bf16_t*)y1; a.res = (const convk::bf16_t*)residual; a.out = (convk::bf16_t*)out; a.y1n = (convk::bf16_t*)y1_next;
    a.wstream = (const uint4*)p->wstream;
    a.sc2 = p->scale2; a.sh2 = p->shift2; a.sc3 = p->scale3; a.sh3 = p->shift3; a.sc1n = p->scale1n; a.sh1n = p->shift1n;
    a.H = H; a.tiles_per_img = H / 4; a.ntiles = B * (H / 4);
    const int grid = persistent_grid(a.ntiles);
    hipStream_t s = (hipStream_t)stream;
    const bool f16 = p->dtype == DIR_DT_F16;
    if (p->n_next == 256) {
        if (f16) DIR_LAUNCH((l3_chain_kernel<256, f16s_t>), dim3(grid), dim3(NTHR), 0, s, a);
        else DIR_LAUNCH((l3_chain_kernel<256, bf16_t>), dim3(grid), dim3(NTHR), 0, s, a);
    } else {
        if (f16) DIR_LAUNCH((l3_chain_kernel<0, f16s_t>), dim3(grid), dim3(NTHR), 0, s, a);
        else DIR_LAUNCH((l3_chain_kernel<0, bf16_t>), dim3(grid), dim3(NTHR), 0, s, a);
    }
    return check_launch("dir_bottleneck_block_forward");
}
