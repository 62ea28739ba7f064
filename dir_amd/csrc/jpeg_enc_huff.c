/* Host half of the JPEG ENCODE path: the ENTROPY CODING of a coefficient record and the file syntax -- and nothing else.
 *
 *   reference   dataset/prepare_data.py:174-214  cv.imwrite(<split>/mask/<idx>.jpg), cv.imwrite(<split>/dense/<idx>.jpg)
 *               (OpenCV's bundled libjpeg-turbo: RGB -> YCbCr, h2v2 downsampling, islow forward DCT, quantisation -> Huffman coding with the
 *               Annex K tables -> a baseline JFIF file)
 *
 * The mirror image of jpeg_huff.c: everything before the Huffman coder is integer arithmetic on independent MCUs and runs on the GPU
 * (csrc/jpeg_enc.hip: dir_jpeg_encode_records writes the same record format dir_jpeg_decode_coefficients produces); the bit stream is serial
 * and stays on the host.  The file layout (include/dir_jpeg_enc.h) is libjpeg's default one, so a record made at quality q becomes the bytes
 * libjpeg-turbo writes for the frame at quality q (tests/test_jpeg_enc_ref.py pins that to files Pillow wrote).
 *
 * Generic over what the header describes (1 or 3 components; 4:4:4, 4:2:2, 4:2:0): any record the decoder produces can be written back.
 * Plain C (gcc), no dependencies, no global state: the code tables are derived per call on the stack. */
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/dir_jpeg_enc.h"

static const uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

/* ITU T.81 Annex K.1: the example quantisation tables (natural order) that jpeg_set_quality scales */
static const uint8_t kBaseLuma[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
                                      18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,  49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
static const uint8_t kBaseChroma[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
                                        99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};

/* ITU T.81 Annex K.3: the typical Huffman tables (code counts per length 1..16, symbols in code order) */
static const uint8_t kDcLumaBits[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
static const uint8_t kDcLumaVals[12] = {0x00, 0x01, 0x02, 0x03, 0x04, 0x05, 0x06, 0x07, 0x08, 0x09, 0x0a, 0x0b};
static const uint8_t kAcLumaBits[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125};
static const uint8_t kAcLumaVals[162] = {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08,
    0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
    0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
    0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
    0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
    0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
static const uint8_t kDcChromaBits[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
static const uint8_t kDcChromaVals[12] = {0x00, 0x01, 0x02, 0x03, 0x04, 0x05, 0x06, 0x07, 0x08, 0x09, 0x0a, 0x0b};
static const uint8_t kAcChromaBits[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119};
static const uint8_t kAcChromaVals[162] = {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
    0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
    0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
    0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
    0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};

typedef struct {
    uint16_t code[256];
    uint8_t size[256]; /* 0: the symbol has no code */
} ehuff_t;

static void build_ehuff(ehuff_t* e, const uint8_t* counts, const uint8_t* symbols) {
    memset(e, 0, sizeof(*e));
    unsigned code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < counts[len - 1]; ++i, ++k, ++code) {
            e->code[symbols[k]] = (uint16_t)code;
            e->size[symbols[k]] = (uint8_t)len;
        }
        code <<= 1;
    }
}

typedef struct {
    uint8_t* p;
    uint8_t* end;
    uint64_t acc; /* the low `n` bits are pending */
    int n;
    int full; /* a byte did not fit: nothing is written from here on */
} bitw_t;

static inline void put_byte(bitw_t* b, unsigned v) {
    if (b->p < b->end) *b->p++ = (uint8_t)v;
    else b->full = 1;
}
static inline void put_bits(bitw_t* b, unsigned code, int size) { /* size <= 16 + 11; fewer than 32 bits are pending on entry */
    b->acc = (b->acc << size) | code;
    b->n += size;
    if (b->n < 32) return;
    const uint32_t w = (uint32_t)(b->acc >> (b->n - 32));
    /* four bytes at once when none of them is 0xFF (no byte of ~w is zero) and they fit */
    if (!((~w - 0x01010101u) & w & 0x80808080u) && b->end - b->p >= 4) {
        b->p[0] = (uint8_t)(w >> 24); b->p[1] = (uint8_t)(w >> 16); b->p[2] = (uint8_t)(w >> 8); b->p[3] = (uint8_t)w;
        b->p += 4;
        b->n -= 32;
        return;
    }
    while (b->n >= 8) {
        const unsigned byte = (unsigned)(b->acc >> (b->n - 8)) & 0xffu;
        put_byte(b, byte);
        if (byte == 0xff) put_byte(b, 0); /* byte stuffing */
        b->n -= 8;
    }
}
static inline void flush_bits(bitw_t* b) { /* the whole bytes that are pending, then 1 bits up to the next byte boundary */
    if (b->n & 7) {
        const int pad = 8 - (b->n & 7);
        b->acc = (b->acc << pad) | ((1u << pad) - 1u);
        b->n += pad;
    }
    while (b->n >= 8) {
        const unsigned byte = (unsigned)(b->acc >> (b->n - 8)) & 0xffu;
        put_byte(b, byte);
        if (byte == 0xff) put_byte(b, 0);
        b->n -= 8;
    }
}
static inline int bit_length(unsigned v) { return v ? 32 - __builtin_clz(v) : 0; }

static void put_marker(bitw_t* b, unsigned m, unsigned len) { /* len: the segment length field (0: a stand-alone marker) */
    put_byte(b, 0xff);
    put_byte(b, m);
    if (len) {
        put_byte(b, len >> 8);
        put_byte(b, len & 0xff);
    }
}
static void put_dht(bitw_t* b, unsigned tc_th, const uint8_t* counts, const uint8_t* symbols) {
    int ns = 0;
    for (int k = 0; k < 16; ++k) ns += counts[k];
    put_marker(b, 0xc4, (unsigned)(2 + 1 + 16 + ns));
    put_byte(b, tc_th);
    for (int k = 0; k < 16; ++k) put_byte(b, counts[k]);
    for (int k = 0; k < ns; ++k) put_byte(b, symbols[k]);
}

/* the header as jpeg_huff.c writes it and jpeg.hip's record_ok reads it: every derived field must be the one width / height / sampling imply */
static int header_ok(const dir_jpeg_header* H, size_t record_bytes, int* unsupported) {
    *unsupported = 0;
    if (H->magic != DIR_JPEG_MAGIC || (H->ncomp != 1 && H->ncomp != 3)) return 0;
    if (H->width < 1 || H->width > 65535 || H->height < 1 || H->height > 65535) return 0;
    const int hm = H->hmax, vm = H->vmax;
    if (!((hm == 1 && vm == 1) || (hm == 2 && vm == 1) || (hm == 2 && vm == 2))) return 0;
    if (H->h[0] != hm || H->v[0] != vm || (H->ncomp == 1 && hm != 1)) return 0;
    const int mcux = (H->width + 8 * hm - 1) / (8 * hm), mcuy = (H->height + 8 * vm - 1) / (8 * vm);
    if (H->mcux != mcux || H->mcuy != mcuy) return 0;
    int64_t total = 0;
    for (int c = 0; c < H->ncomp; ++c) {
        if (c > 0 && (H->h[c] != 1 || H->v[c] != 1)) return 0;
        if (H->blocks_x[c] != mcux * H->h[c] || H->blocks_y[c] != mcuy * H->v[c] || H->coef_offset[c] != total) return 0;
        total += (int64_t)H->blocks_x[c] * H->blocks_y[c] * 64;
    }
    if (total > 0x7fffffffll || total != H->total_coef) return 0;
    if (sizeof(dir_jpeg_header) + (uint64_t)total * 2 > (uint64_t)record_bytes) return 0;
    for (int c = 0; c < H->ncomp; ++c)
        for (int k = 0; k < 64; ++k) {
            if (H->quant[c][k] == 0) return 0;
            if (H->quant[c][k] > 255) *unsupported = 1;
        }
    return 1;
}

size_t dir_jpeg_encode_bound(const void* record, size_t record_bytes) {
    int uns;
    if (!record || record_bytes < sizeof(dir_jpeg_header)) return 0;
    dir_jpeg_header H;
    memcpy(&H, record, sizeof(H));
    if (!header_ok(&H, record_bytes, &uns) || uns) return 0;
    /* markers and tables: < 1 KiB.  A block: at most 27 bits of DC and 63 x 26 bits of AC = 1665 bits < 209 bytes, every one of which may be stuffed */
    return 1024 + (size_t)(H.total_coef / 64) * 420;
}

int dir_jpeg_encode_record(const void* record, size_t record_bytes, uint8_t* out, size_t cap, size_t* n_out) {
    if (!record || !out || !n_out || record_bytes < sizeof(dir_jpeg_header)) return DIR_JPEG_E_ARG;
    *n_out = 0;
    dir_jpeg_header Hc;
    memcpy(&Hc, record, sizeof(Hc)); /* (a record need not be aligned) */
    const dir_jpeg_header* H = &Hc;
    int uns;
    if (!header_ok(H, record_bytes, &uns)) return DIR_JPEG_E_FORMAT;
    if (uns) return DIR_JPEG_E_UNSUPPORTED;
    const int nc = H->ncomp;
    int tq[3] = {0, 1, 1};
    if (nc == 3 && memcmp(H->quant[2], H->quant[1], sizeof(H->quant[1])) != 0) tq[2] = 2;
    const int ntab = nc == 1 ? 1 : tq[2] + 1;

    bitw_t b = {out, out + cap, 0, 0, 0};
    put_marker(&b, 0xd8, 0);
    put_marker(&b, 0xe0, 16);
    static const uint8_t jfif[14] = {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
    for (int k = 0; k < 14; ++k) put_byte(&b, jfif[k]);
    for (int t = 0; t < ntab; ++t) {
        put_marker(&b, 0xdb, 67);
        put_byte(&b, (unsigned)t);
        for (int k = 0; k < 64; ++k) put_byte(&b, H->quant[t][kZigzag[k]]);
    }
    put_marker(&b, 0xc0, (unsigned)(8 + 3 * nc));
    put_byte(&b, 8);
    put_byte(&b, (unsigned)H->height >> 8);
    put_byte(&b, (unsigned)H->height & 0xff);
    put_byte(&b, (unsigned)H->width >> 8);
    put_byte(&b, (unsigned)H->width & 0xff);
    put_byte(&b, (unsigned)nc);
    for (int c = 0; c < nc; ++c) {
        put_byte(&b, (unsigned)(c + 1));
        put_byte(&b, (unsigned)((H->h[c] << 4) | H->v[c]));
        put_byte(&b, (unsigned)tq[c]);
    }
    ehuff_t dc[2], ac[2];
    build_ehuff(&dc[0], kDcLumaBits, kDcLumaVals);
    build_ehuff(&ac[0], kAcLumaBits, kAcLumaVals);
    put_dht(&b, 0x00, kDcLumaBits, kDcLumaVals);
    put_dht(&b, 0x10, kAcLumaBits, kAcLumaVals);
    if (nc == 3) {
        build_ehuff(&dc[1], kDcChromaBits, kDcChromaVals);
        build_ehuff(&ac[1], kAcChromaBits, kAcChromaVals);
        put_dht(&b, 0x01, kDcChromaBits, kDcChromaVals);
        put_dht(&b, 0x11, kAcChromaBits, kAcChromaVals);
    }
    put_marker(&b, 0xda, (unsigned)(6 + 2 * nc));
    put_byte(&b, (unsigned)nc);
    for (int c = 0; c < nc; ++c) {
        put_byte(&b, (unsigned)(c + 1));
        put_byte(&b, c ? 0x11 : 0x00);
    }
    put_byte(&b, 0);
    put_byte(&b, 63);
    put_byte(&b, 0);
    if (b.full) return DIR_JPEG_E_SPACE;

    const char* coef = (const char*)record + sizeof(dir_jpeg_header);
    int pred[3] = {0, 0, 0};
    for (int my = 0; my < H->mcuy; ++my) {
        for (int mx = 0; mx < H->mcux; ++mx) {
            for (int c = 0; c < nc; ++c) {
                const ehuff_t* hd = &dc[c ? 1 : 0];
                const ehuff_t* ha = &ac[c ? 1 : 0];
                for (int by = 0; by < H->v[c]; ++by) {
                    for (int bx = 0; bx < H->h[c]; ++bx) {
                        int16_t blk[64];
                        memcpy(blk, coef + 2 * ((size_t)H->coef_offset[c] + ((size_t)(my * H->v[c] + by) * (size_t)H->blocks_x[c] + (size_t)(mx * H->h[c] + bx)) * 64), sizeof(blk));
                        int v = blk[0] - pred[c];
                        pred[c] = blk[0];
                        int nb = bit_length((unsigned)(v < 0 ? -v : v));
                        if (nb > 11) return DIR_JPEG_E_FORMAT; /* 8-bit baseline: DC difference categories 0..11 (T.81 F.1.2.1.1) */
                        put_bits(&b, ((unsigned)hd->code[nb] << nb) | ((unsigned)(v < 0 ? v - 1 : v) & ((1u << nb) - 1u)), hd->size[nb] + nb);
                        /* the non-zero AC coefficients as a bit mask in zigzag order: rendered frames are mostly empty blocks */
                        uint64_t nz = 0, any = 0, w8[16];
                        memcpy(w8, blk, sizeof(w8));
                        for (int k = 1; k < 16; ++k) any |= w8[k];
                        blk[0] = 0;
                        memcpy(w8, blk, 8);
                        if (any | w8[0])
                            for (int k = 1; k < 64; ++k) nz |= (uint64_t)(blk[kZigzag[k]] != 0) << k;
                        int last = 0;
                        while (nz) {
                            const int k = __builtin_ctzll(nz);
                            nz &= nz - 1;
                            int run = k - last - 1;
                            last = k;
                            for (; run > 15; run -= 16) put_bits(&b, ha->code[0xf0], ha->size[0xf0]); /* ZRL */
                            v = blk[kZigzag[k]];
                            nb = bit_length((unsigned)(v < 0 ? -v : v));
                            if (nb > 10) return DIR_JPEG_E_FORMAT; /* AC categories 1..10 (T.81 F.1.2.2.1) */
                            const int sym = (run << 4) | nb;
                            put_bits(&b, ((unsigned)ha->code[sym] << nb) | ((unsigned)(v < 0 ? v - 1 : v) & ((1u << nb) - 1u)), ha->size[sym] + nb);
                        }
                        if (last != 63) put_bits(&b, ha->code[0x00], ha->size[0x00]); /* EOB */
                        if (b.full) return DIR_JPEG_E_SPACE;
                    }
                }
            }
        }
    }
    flush_bits(&b); /* the last byte is padded with 1 bits */
    put_marker(&b, 0xd9, 0);
    if (b.full) return DIR_JPEG_E_SPACE;
    *n_out = (size_t)(b.p - out);
    return DIR_JPEG_OK;
}

int dir_jpeg_quality_tables(int quality, uint16_t luma[64], uint16_t chroma[64]) {
    if (!luma || !chroma || quality < 1 || quality > 100) return DIR_JPEG_E_ARG;
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int k = 0; k < 64; ++k) {
        int l = (kBaseLuma[k] * s + 50) / 100, c = (kBaseChroma[k] * s + 50) / 100;
        luma[k] = (uint16_t)(l < 1 ? 1 : l > 255 ? 255 : l);
        chroma[k] = (uint16_t)(c < 1 ? 1 : c > 255 ? 255 : c);
    }
    return DIR_JPEG_OK;
}

int dir_jpeg_enc_abi_version(void) { return DIR_JPEG_ENC_ABI_VERSION; }
