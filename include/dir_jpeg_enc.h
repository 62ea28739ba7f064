/* libdir_jpeg.so -- the HOST half of the JPEG ENCODE path: a coefficient record (include/dir_jpeg.h: dir_jpeg_header + quantised int16
 * coefficients) -> the bytes of a baseline JFIF file.  The mirror image of dir_jpeg_decode_coefficients: Huffman coding with the Annex K tables
 * and the file syntax, nothing else; the GPU half (dir_jpeg_encode_records in dir_hip.h) does colour conversion, chroma downsampling, forward
 * DCT and quantisation.  Plain C ABI, no GPU runtime (the encode worker processes of dir_amd.apps.render_split load it).
 *
 * Replaces, together with dir_jpeg_encode_records, the  cv.imwrite(<split>/mask|dense/<idx>.jpg)  of dataset/prepare_data.py:174-214: a 4:2:0
 * record made by dir_jpeg_encode_records at quality q is written as the file libjpeg(-turbo) writes for the same frame at quality q with its
 * default settings (Pillow's Image.save(format='JPEG', quality=q, subsampling=2)), byte for byte.
 *
 * The file:  SOI | APP0 "JFIF\0" 1.01, units 0, density 1x1, no thumbnail | DQT table 0 | DQT table 1 (one segment each, 8-bit, zigzag order;
 * grayscale: table 0 only; a third table only when Cr's differs from Cb's) | SOF0 precision 8, height, width, components (1, HV, 0) (2, 0x11, 1)
 * (3, 0x11, 1) | DHT DC 0 | DHT AC 0 | DHT DC 1 | DHT AC 1 (one segment each, the Annex K tables; grayscale: the first two) | SOS (1, 0x00)
 * (2, 0x11) (3, 0x11), Ss 0, Se 63, AhAl 0 | one interleaved scan, per MCU the luma blocks in raster order then Cb then Cr, DC prediction per
 * component, no restart markers, 0x00 stuffed after every 0xFF, the last byte padded with 1 bits | EOI.
 *
 * This header has its own version: include/dir_jpeg.h and its DIR_JPEG_ABI_VERSION are unchanged by it.  The error codes and the record are
 * dir_jpeg.h's. */
#ifndef DIR_JPEG_ENC_H_
#define DIR_JPEG_ENC_H_
#include <stddef.h>
#include <stdint.h>

#include "dir_jpeg.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DIR_JPEG_ENC_ABI_VERSION 1

/* record (header + coefficients, as dir_jpeg_decode_coefficients or dir_jpeg_encode_records wrote it: 1 or 3 components, 4:4:4, 4:2:2 or 4:2:0)
 * -> out[0 .. *n_out).  The header is validated before any field is trusted (geometry consistent with width / height / sampling factors,
 * record_bytes holds total_coef, table entries 1..255).  Never writes past out + cap.  Returns DIR_JPEG_OK, or
 *   DIR_JPEG_E_ARG          null pointer / record smaller than a header
 *   DIR_JPEG_E_FORMAT       not a coefficient record, inconsistent header, or a coefficient baseline Huffman coding cannot carry
 *                           (|AC| > 1023, |DC difference| > 2047): no wrong code is emitted
 *   DIR_JPEG_E_UNSUPPORTED  a quantisation entry above 255 (would need a 16-bit DQT, which a baseline file may not carry)
 *   DIR_JPEG_E_SPACE        cap is too small (dir_jpeg_encode_bound always suffices)
 * Thread-safe, no global state. */
int dir_jpeg_encode_record(const void* record, size_t record_bytes, uint8_t* out, size_t cap, size_t* n_out);
/* a cap that always suffices for this record; 0 if the record is not one dir_jpeg_encode_record accepts */
size_t dir_jpeg_encode_bound(const void* record, size_t record_bytes);
/* libjpeg's jpeg_set_quality(quality, force_baseline = TRUE): s = 5000 / q for q < 50, else 200 - 2 q; entry = clamp((base * s + 50) / 100, 1, 255)
 * over the Annex K luminance / chrominance tables.  Natural (row-major) order.  quality outside 1..100: DIR_JPEG_E_ARG. */
int dir_jpeg_quality_tables(int quality, uint16_t luma[64], uint16_t chroma[64]);
int dir_jpeg_enc_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif
