// dir_jpeg_encode_records: the GPU half of the JPEG ENCODE path -- the mirror image of dir_jpeg_decode_records (csrc/jpeg.hip).
//
//   reference   dataset/prepare_data.py:174-214  cv.imwrite(<split>/mask/<idx>.jpg, ...), cv.imwrite(<split>/dense/<idx>.jpg, ...)
//               = libjpeg's default compression: RGB -> YCbCr (jccolor.c), h2v2 chroma downsampling (jcsample.c), the "islow" forward DCT
//               (jfdctint.c), quantisation (jcdctmgr.c) -> Huffman coding + file syntax
//
// Everything before the Huffman coder runs here, in one launch: uint8 frames [B,H,W,3] -> one RECORD per image (a 512-byte dir_jpeg_header +
// the quantised int16 coefficients, the format dir_jpeg_decode_coefficients defines); the host writes the bit stream (csrc/jpeg_enc_huff.c).
// Integer arithmetic throughout (int32: tests/test_jpeg_enc_ref.py holds every intermediate of saturated frames inside it), BIT-EXACT with
// libjpeg-turbo: the rule is written out in include/dir_hip.h, restated in tests/helpers/jpeg_enc_ref.py and pinned to files Pillow wrote.
//
//   jpeg_encode_kernel   one workgroup of 256 threads per FOUR MCUs (consecutive in the image's raster order of MCUs); an MCU depends on nothing
//                        but its own 16 x 16 pixels, so there are no atomics, no scratch and no workspace, and an image gives the same bytes
//                        in any slot of any batch.
//     1  load + colour   every thread loads three aligned dwords = four pixels of one MCU row (a wave reads one MCU: 16 rows x 48 contiguous
//                        bytes), converts them and leaves in LDS Y - 128 (int16) and the horizontal pair sums of Cb and Cr (int16)
//     2  row DCT         192 threads, one per (MCU, block, row): eight samples from LDS (chroma: two rows of pair sums + the alternating bias,
//                        >> 2, - 128), the butterfly fully unrolled on named registers, eight int32 back to LDS (block pitch 72 dwords: the
//                        column pass of 8 blocks x 8 columns then reads 64 distinct banks)
//     3  column DCT      192 threads, one per (MCU, block, column): the butterfly, quantisation by an exact reciprocal (below), int16 to LDS
//     4  store           192 threads, one uint4 (a block row of eight coefficients) each: a block is 128 contiguous bytes, the two luma blocks
//                        of an MCU row 256, whole dwords only.  The group that holds an image's first MCU also writes its header.
//
// Quantisation  sign(c) (|c| + (8q >> 1)) / (8q)  without a division: with d = 8q <= 2040 and m = floor((2^32 - 1) / d) + 1 = ceil(2^32 / d),
// floor(n / d) == umulhi(n, m) for every n with n (m d - 2^32) < 2^32; m d - 2^32 < d < 2^11 and n = |c| + 4q < 2^21 (|c| <= 2^16 after the
// DCT of 8-bit samples), so the product stays below 2^32 and the integers are the division's.  The 128 reciprocals are made on the host and
// travel in the kernel arguments, like the header; so does the reciprocal of the MCUs per row (MCU index < 2^16, divisor <= 2^8: exact by the
// same bound), which leaves the kernel without an integer division.
#include "dir_common.h"

#include <string.h>

#include "../../include/dir_jpeg.h"

namespace {

constexpr int MCUS = 4;        // MCUs per workgroup
constexpr int WS_PITCH = 72;   // int32 per block in the row-pass workspace (64 + 8)

struct JpegEncArgs {
    dir_jpeg_header hdr;        // the header every record gets (quant[0] luma, quant[1] = quant[2] chroma), made on the host
    const unsigned char* frames;
    char* records;
    long long stride;
    int H, W, rgb;              // rgb 0: the frames are B, G, R; 1: R, G, B
    int mcux, nmcu;             // MCUs per row / per image
    unsigned mcux_recip;        // ceil(2^32 / mcux); not used for mcux == 1, where 2^32 does not fit
    unsigned recip[128];        // ceil(2^32 / (8 q)) for the luma, then the chroma table
};

// jfdctint.c: one pass over eight values.  PASS1: rows (outputs scaled up by PASS1_BITS); else columns (scaled down again, + the factor 8)
template <bool PASS1>
__device__ __forceinline__ void fdct8(int d0, int d1, int d2, int d3, int d4, int d5, int d6, int d7, int& o0, int& o1, int& o2, int& o3, int& o4,
                                      int& o5, int& o6, int& o7) {
    constexpr int F_0_298631336 = 2446, F_0_390180644 = 3196, F_0_541196100 = 4433, F_0_765366865 = 6270, F_0_899976223 = 7373, F_1_175875602 = 9633,
                  F_1_501321110 = 12299, F_1_847759065 = 15137, F_1_961570560 = 16069, F_2_053119869 = 16819, F_2_562915447 = 20995,
                  F_3_072711026 = 25172;
    constexpr int SH = PASS1 ? 11 : 15, HALF = 1 << (SH - 1);      // CONST_BITS -/+ PASS1_BITS
    const int tmp0 = d0 + d7, tmp7 = d0 - d7, tmp1 = d1 + d6, tmp6 = d1 - d6, tmp2 = d2 + d5, tmp5 = d2 - d5, tmp3 = d3 + d4, tmp4 = d3 - d4;
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    if (PASS1) {
        o0 = (tmp10 + tmp11) * 4;
        o4 = (tmp10 - tmp11) * 4;
    } else {
        o0 = (tmp10 + tmp11 + 2) >> 2;
        o4 = (tmp10 - tmp11 + 2) >> 2;
    }
    // every factor is below 2^23 in magnitude (8-bit samples: |pass-2 input| < 2^15, sums of four < 2^17; constants < 2^15) and every product
    // inside int32, so the 24-bit multiplier (full rate) gives the 32-bit product
    int z1 = __mul24(tmp12 + tmp13, F_0_541196100);
    o2 = (z1 + __mul24(tmp13, F_0_765366865) + HALF) >> SH;
    o6 = (z1 - __mul24(tmp12, F_1_847759065) + HALF) >> SH;
    z1 = tmp4 + tmp7;
    int z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
    const int z5 = __mul24(z3 + z4, F_1_175875602);
    const int t4 = __mul24(tmp4, F_0_298631336), t5 = __mul24(tmp5, F_2_053119869), t6 = __mul24(tmp6, F_3_072711026), t7 = __mul24(tmp7, F_1_501321110);
    z1 = __mul24(z1, -F_0_899976223);
    z2 = __mul24(z2, -F_2_562915447);
    z3 = __mul24(z3, -F_1_961570560) + z5;
    z4 = __mul24(z4, -F_0_390180644) + z5;
    o7 = (t4 + z1 + z3 + HALF) >> SH;
    o5 = (t5 + z2 + z4 + HALF) >> SH;
    o3 = (t6 + z2 + z3 + HALF) >> SH;
    o1 = (t7 + z1 + z4 + HALF) >> SH;
}

__device__ __forceinline__ int lo16(unsigned v) { return (int)(short)(v & 0xffffu); }
__device__ __forceinline__ int hi16(unsigned v) { return (int)v >> 16; }
__device__ __forceinline__ unsigned pack16(int a, int b) { return ((unsigned)a & 0xffffu) | ((unsigned)b << 16); }

__device__ __forceinline__ unsigned quant1(int c, unsigned q4, unsigned m) {      // q4 = 8q >> 1; -> the low 16 bits of the int16 result
    const unsigned n = (unsigned)(c < 0 ? -c : c) + q4;
    const int r = (int)__umulhi(n, m);
    return (unsigned)(c < 0 ? -r : r) & 0xffffu;
}

__global__ __launch_bounds__(256) void jpeg_encode_kernel(const JpegEncArgs a) {
    __shared__ __attribute__((aligned(16))) short s_y[MCUS][16][16];      // Y - 128
    __shared__ __attribute__((aligned(16))) short s_c[MCUS][2][16][8];    // Cb, Cr: sums of horizontal pixel pairs
    __shared__ __attribute__((aligned(16))) int s_ws[MCUS * 6][WS_PITCH];  // after the row pass
    __shared__ __attribute__((aligned(16))) short s_q[MCUS * 6][64];      // quantised
    __shared__ unsigned s_recip[128];
    __shared__ unsigned s_half[128];

    const int t = threadIdx.x;
    const int img = blockIdx.y, grp = blockIdx.x;
    char* rec = a.records + (long long)img * a.stride;
    if (t < 128) {
        const unsigned q = a.hdr.quant[t >> 6][t & 63];                    // [0]: luma, [1]: chroma
        s_recip[t] = a.recip[t];
        s_half[t] = 4u * q;
        if (grp == 0) reinterpret_cast<unsigned*>(rec)[t] = reinterpret_cast<const unsigned*>(&a.hdr)[t];
    }

    // ---- 1: four pixels of one MCU row per thread
    {
        const int m = t >> 6, l = t & 63, r = l >> 2, q = l & 3;
        const int mcu = grp * MCUS + m;
        if (mcu < a.nmcu) {
            const int my = a.mcux == 1 ? mcu : (int)__umulhi((unsigned)mcu, a.mcux_recip), mx = mcu - my * a.mcux;
            const unsigned* src = reinterpret_cast<const unsigned*>(a.frames + ((long long)img * a.H * a.W + (long long)(my * 16 + r) * a.W + mx * 16 + q * 4) * 3);
            const unsigned w0 = src[0], w1 = src[1], w2 = src[2];
            const int c0[4] = {(int)(w0 & 255u), (int)(w0 >> 24), (int)((w1 >> 16) & 255u), (int)((w2 >> 8) & 255u)};       // first channel of the four pixels
            const int c1[4] = {(int)((w0 >> 8) & 255u), (int)(w1 & 255u), (int)(w1 >> 24), (int)((w2 >> 16) & 255u)};
            const int c2[4] = {(int)((w0 >> 16) & 255u), (int)((w1 >> 8) & 255u), (int)(w2 & 255u), (int)(w2 >> 24)};
            int Y[4], Cb[4], Cr[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int R = a.rgb ? c0[e] : c2[e], G = c1[e], B = a.rgb ? c2[e] : c0[e];
                // jccolor.c: FIX(x) = int(x * 65536 + 0.5); ONE_HALF = 32768; CBCR_OFFSET = 128 << 16
                Y[e] = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16;
                Cb[e] = (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16;
                Cr[e] = (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16;
            }
            uint2 yy;
            yy.x = pack16(Y[0] - 128, Y[1] - 128);
            yy.y = pack16(Y[2] - 128, Y[3] - 128);
            *reinterpret_cast<uint2*>(&s_y[m][r][q * 4]) = yy;
            *reinterpret_cast<unsigned*>(&s_c[m][0][r][q * 2]) = pack16(Cb[0] + Cb[1], Cb[2] + Cb[3]);
            *reinterpret_cast<unsigned*>(&s_c[m][1][r][q * 2]) = pack16(Cr[0] + Cr[1], Cr[2] + Cr[3]);
        }
    }
    __syncthreads();

    // ---- 2 .. 4: one thread per (MCU, block, row / column)
    const int m = t / 48, j = t - m * 48, b = j >> 3, k = j & 7;            // t < 192: m < 4
    const bool live = t < MCUS * 48 && grp * MCUS + m < a.nmcu;
    const int blk = m * 6 + b;
    if (live) {
        int d0, d1, d2, d3, d4, d5, d6, d7;
        if (b < 4) {
            const uint4 v = *reinterpret_cast<const uint4*>(&s_y[m][(b >> 1) * 8 + k][(b & 1) * 8]);
            d0 = lo16(v.x); d1 = hi16(v.x); d2 = lo16(v.y); d3 = hi16(v.y); d4 = lo16(v.z); d5 = hi16(v.z); d6 = lo16(v.w); d7 = hi16(v.w);
        } else {
            // jcsample.c h2v2_downsample: (the four pixels + bias) >> 2, bias 1 for even output columns, 2 for odd ones
            const uint4 u = *reinterpret_cast<const uint4*>(&s_c[m][b - 4][2 * k][0]);
            const uint4 v = *reinterpret_cast<const uint4*>(&s_c[m][b - 4][2 * k + 1][0]);
            d0 = ((lo16(u.x) + lo16(v.x) + 1) >> 2) - 128; d1 = ((hi16(u.x) + hi16(v.x) + 2) >> 2) - 128;
            d2 = ((lo16(u.y) + lo16(v.y) + 1) >> 2) - 128; d3 = ((hi16(u.y) + hi16(v.y) + 2) >> 2) - 128;
            d4 = ((lo16(u.z) + lo16(v.z) + 1) >> 2) - 128; d5 = ((hi16(u.z) + hi16(v.z) + 2) >> 2) - 128;
            d6 = ((lo16(u.w) + lo16(v.w) + 1) >> 2) - 128; d7 = ((hi16(u.w) + hi16(v.w) + 2) >> 2) - 128;
        }
        int4 lo, hi;
        fdct8<true>(d0, d1, d2, d3, d4, d5, d6, d7, lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w);
        *reinterpret_cast<int4*>(&s_ws[blk][k * 8]) = lo;
        *reinterpret_cast<int4*>(&s_ws[blk][k * 8 + 4]) = hi;
    }
    __syncthreads();
    if (live) {
        int o0, o1, o2, o3, o4, o5, o6, o7;
        fdct8<false>(s_ws[blk][k], s_ws[blk][8 + k], s_ws[blk][16 + k], s_ws[blk][24 + k], s_ws[blk][32 + k], s_ws[blk][40 + k], s_ws[blk][48 + k],
                     s_ws[blk][56 + k], o0, o1, o2, o3, o4, o5, o6, o7);
        const int tb = (b < 4 ? 0 : 64) + k;
        s_q[blk][k] = (short)quant1(o0, s_half[tb], s_recip[tb]);
        s_q[blk][8 + k] = (short)quant1(o1, s_half[tb + 8], s_recip[tb + 8]);
        s_q[blk][16 + k] = (short)quant1(o2, s_half[tb + 16], s_recip[tb + 16]);
        s_q[blk][24 + k] = (short)quant1(o3, s_half[tb + 24], s_recip[tb + 24]);
        s_q[blk][32 + k] = (short)quant1(o4, s_half[tb + 32], s_recip[tb + 32]);
        s_q[blk][40 + k] = (short)quant1(o5, s_half[tb + 40], s_recip[tb + 40]);
        s_q[blk][48 + k] = (short)quant1(o6, s_half[tb + 48], s_recip[tb + 48]);
        s_q[blk][56 + k] = (short)quant1(o7, s_half[tb + 56], s_recip[tb + 56]);
    }
    __syncthreads();
    if (live) {
        const int mcu = grp * MCUS + m;
        const int my = a.mcux == 1 ? mcu : (int)__umulhi((unsigned)mcu, a.mcux_recip), mx = mcu - my * a.mcux;
        // block index inside the record: Y [2 mcuy][2 mcux], then Cb [mcuy][mcux], then Cr
        const int bi = b < 4 ? ((my * 2 + (b >> 1)) * (a.mcux * 2) + mx * 2 + (b & 1)) : (4 + (b - 4)) * a.nmcu + mcu;
        short* dst = reinterpret_cast<short*>(rec + sizeof(dir_jpeg_header)) + (long long)bi * 64 + k * 8;
        *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(&s_q[blk][k * 8]);
    }
}

}  // namespace

extern "C" int dir_jpeg_encode_records(const void* frames, int B, int H, int W, int channel_order, const uint16_t* luma_q, const uint16_t* chroma_q,
                                       void* records, long long record_stride, void* stream) {
    DIR_REQUIRE(frames && records && luma_q && chroma_q && B >= 0, "dir_jpeg_encode_records: bad arguments");
    DIR_REQUIRE(H > 0 && W > 0 && H % 16 == 0 && W % 16 == 0 && H <= 4096 && W <= 4096,
                "dir_jpeg_encode_records: %d x %d frames: height and width must be multiples of 16 (whole MCUs), at most 4096", H, W);
    DIR_REQUIRE(channel_order == 0 || channel_order == 1, "dir_jpeg_encode_records: channel_order %d (0 = BGR, 1 = RGB)", channel_order);
    for (int k = 0; k < 64; ++k)
        DIR_REQUIRE(luma_q[k] >= 1 && luma_q[k] <= 255 && chroma_q[k] >= 1 && chroma_q[k] <= 255,
                    "dir_jpeg_encode_records: quantisation entry %d is %d / %d: a baseline table holds 1..255", k, (int)luma_q[k], (int)chroma_q[k]);
    const int mcux = W / 16, mcuy = H / 16, nmcu = mcux * mcuy;
    const long long need = (long long)sizeof(dir_jpeg_header) + (long long)nmcu * 6 * 128;
    DIR_REQUIRE(record_stride >= need && record_stride % 16 == 0, "dir_jpeg_encode_records: record_stride %lld: at least %lld bytes (dir_jpeg_record_bytes) and a multiple of 16",
                record_stride, need);
    DIR_REQUIRE(((uintptr_t)records & 15) == 0 && ((uintptr_t)frames & 3) == 0, "dir_jpeg_encode_records: records must be 16-byte aligned, frames 4-byte aligned");
    const int groups = (nmcu + MCUS - 1) / MCUS;
    if (B == 0) return DIR_OK;
    JpegEncArgs a;
    memset(&a.hdr, 0, sizeof(a.hdr));
    a.hdr.magic = DIR_JPEG_MAGIC; a.hdr.width = W; a.hdr.height = H; a.hdr.ncomp = 3;
    a.hdr.hmax = 2; a.hdr.vmax = 2; a.hdr.mcux = mcux; a.hdr.mcuy = mcuy;
    for (int c = 0; c < 3; ++c) {
        a.hdr.h[c] = a.hdr.v[c] = c == 0 ? 2 : 1;
        a.hdr.blocks_x[c] = mcux * a.hdr.h[c];
        a.hdr.blocks_y[c] = mcuy * a.hdr.v[c];
        a.hdr.coef_offset[c] = c == 0 ? 0 : (3 + c) * nmcu * 64;
        memcpy(a.hdr.quant[c], c == 0 ? luma_q : chroma_q, sizeof(a.hdr.quant[c]));
    }
    a.hdr.total_coef = 6 * nmcu * 64;
    a.frames = (const unsigned char*)frames; a.records = (char*)records; a.stride = record_stride;
    a.H = H; a.W = W; a.rgb = channel_order; a.mcux = mcux; a.nmcu = nmcu;
    a.mcux_recip = mcux == 1 ? 0u : 0xffffffffu / (unsigned)mcux + 1u;
    for (int k = 0; k < 128; ++k) a.recip[k] = 0xffffffffu / (8u * (k < 64 ? luma_q[k] : chroma_q[k - 64])) + 1u;
    for (int b0 = 0; b0 < B; b0 += 65535) {                                  // blockIdx.y = the image
        a.frames = (const unsigned char*)frames + (long long)b0 * H * W * 3;
        a.records = (char*)records + (long long)b0 * record_stride;
        DIR_LAUNCH(jpeg_encode_kernel, dim3((unsigned)groups, (unsigned)(B - b0 < 65535 ? B - b0 : 65535)), dim3(256), 0, (hipStream_t)stream, a);
    }
    return dir::check_launch("dir_jpeg_encode_records");
}
