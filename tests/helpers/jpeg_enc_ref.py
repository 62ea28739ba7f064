"""TEST INFRASTRUCTURE: a numpy restatement, in int64, of the baseline JPEG ENCODE the project splits between the GPU
(dir_jpeg_encode_records, csrc/jpeg_enc.hip) and the host (dir_jpeg_encode_record, csrc/jpeg_enc_huff.c) -- libjpeg's default compression
path for a three-component 4:2:0 file, the one cv.imwrite / Pillow run (dataset/prepare_data.py:174-214 writes mask/ and dense/ with it):

    quality tables          jpeg_set_quality(q, force_baseline) over the Annex K tables                         jcparam.c
    colour conversion       RGB -> YCbCr, 16-bit fixed point                                                     jccolor.c
    chroma downsampling     h2v2 box filter with the alternating bias 1, 2, 1, 2, ...                            jcsample.c
    forward DCT             "islow" (CONST_BITS 13, PASS1_BITS 2) on sample - 128: rows, then columns            jfdctint.c
    quantisation            sign(c) * ((|c| + (8q >> 1)) // (8q))                                                jcdctmgr.c
    entropy coding          Huffman with the Annex K tables, one interleaved scan, the JFIF file syntax          jchuff.c, jcmarker.c

The library is a third-party dependency; the algorithm is restated from its published description and PINNED to the bytes Pillow's
libjpeg-turbo wrote (tests/golden/g26_jpeg_enc.npz, tests/test_jpeg_enc_ref.py).  Every intermediate of the DCT is int64 here; `track` collects
the largest magnitude seen, which the tests hold against int32 (the kernel's arithmetic)."""
import numpy as np

from oracle import jpeg as J

MAGIC = 0x4a524944
HEADER_BYTES = 512

BASE_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                      18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99], np.int64)
BASE_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32, np.int64)

# ITU T.81 Annex K.3 (counts per code length 1..16, symbols in code order)
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125], list(bytes.fromhex(
    '01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a434445464748494a53545556'
    '5758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6'
    'd7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa')))
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119], list(bytes.fromhex(
    '000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a434445464748494a535455'
    '565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4'
    'd5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa')))


def quality_tables(q):
    """jpeg_set_quality(q, force_baseline=TRUE) -> (luma [64], chroma [64]) int64, natural order"""
    assert 1 <= q <= 100
    s = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((b * s + 50) // 100, 1, 255) for b in (BASE_LUMA, BASE_CHROMA))


def _fix(x):
    return int(x * 65536 + 0.5)


def rgb_to_ycc(rgb):
    """uint8 [..., 3] RGB -> (Y, Cb, Cr) int64"""
    r, g, b = (rgb[..., k].astype(np.int64) for k in range(3))
    y = (_fix(.299) * r + _fix(.587) * g + _fix(.114) * b + 32768) >> 16
    cb = (-_fix(.16874) * r - _fix(.33126) * g + _fix(.5) * b + (128 << 16) + 32767) >> 16
    cr = (_fix(.5) * r - _fix(.41869) * g - _fix(.08131) * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def downsample_h2v2(p):
    """[H, W] -> [H/2, W/2]: (a + b + c + d + bias) >> 2, bias 1 for even output columns, 2 for odd ones"""
    s = p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2]
    bias = 1 + (np.arange(s.shape[1], dtype=np.int64) & 1)
    return (s + bias[None, :]) >> 2


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_1d(d, first, track):
    """jfdctint.c's butterfly on eight int64 vectors; first=True: pass 1 (rows), else pass 2 (columns)"""
    C, P = J.CONST_BITS, J.PASS1_BITS

    def t(*xs):
        if track is not None:
            for x in xs:
                track[0] = max(track[0], int(np.abs(x).max()))
        return xs[0] if len(xs) == 1 else xs
    tmp0, tmp7, tmp1, tmp6 = t(d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6])
    tmp2, tmp5, tmp3, tmp4 = t(d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4])
    tmp10, tmp13, tmp11, tmp12 = t(tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2)
    o = [None] * 8
    if first:
        o[0], o[4] = t((tmp10 + tmp11) << P, (tmp10 - tmp11) << P)
    else:
        o[0], o[4] = _descale(t(tmp10 + tmp11), P), _descale(t(tmp10 - tmp11), P)
    sh = C - P if first else C + P
    half = 1 << (sh - 1)
    z1 = t((tmp12 + tmp13) * J.F_0_541196100)
    o[2] = t(t(z1 + t(tmp13 * J.F_0_765366865)) + half) >> sh
    o[6] = t(t(z1 + t(tmp12 * (-J.F_1_847759065))) + half) >> sh
    z1, z2, z3, z4 = t(tmp4 + tmp7, tmp5 + tmp6, tmp4 + tmp6, tmp5 + tmp7)
    z5 = t(t(z3 + z4) * J.F_1_175875602)
    tmp4, tmp5, tmp6, tmp7 = t(tmp4 * J.F_0_298631336, tmp5 * J.F_2_053119869, tmp6 * J.F_3_072711026, tmp7 * J.F_1_501321110)
    z1, z2, z3, z4 = t(z1 * (-J.F_0_899976223), z2 * (-J.F_2_562915447), z3 * (-J.F_1_961570560), z4 * (-J.F_0_390180644))
    z3, z4 = t(z3 + z5, z4 + z5)
    o[7] = t(t(t(tmp4 + z1) + z3) + half) >> sh
    o[5] = t(t(t(tmp5 + z2) + z4) + half) >> sh
    o[3] = t(t(t(tmp6 + z2) + z3) + half) >> sh
    o[1] = t(t(t(tmp7 + z1) + z4) + half) >> sh
    return o


def fdct_islow(blocks, track=None):
    """samples - 128 as int64 [..., 8 rows, 8 cols] -> coefficients scaled by 8, [..., 8, 8]; track: [0] -> the largest |intermediate|"""
    rows = _fdct_1d([blocks[..., :, k] for k in range(8)], True, track)
    ws = np.stack(rows, -1)
    cols = _fdct_1d([ws[..., r, :] for r in range(8)], False, track)
    return np.stack(cols, -2)


def quantise(c, q):
    """c [..., 64] scaled by 8, q [64]"""
    d = 8 * q.astype(np.int64)
    return np.sign(c) * ((np.abs(c) + (d >> 1)) // d)


def _blocks(plane):
    """[8 by, 8 bx] plane -> [by, bx, 8, 8]"""
    h, w = plane.shape
    return plane.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)


def coefficients(frame, quality, channel_order='bgr', track=None):
    """uint8 [H, W, 3] (H, W multiples of 16) -> (luma q, chroma q, [Y, Cb, Cr] int16 arrays [blocks_y, blocks_x, 64])"""
    H, W = frame.shape[:2]
    assert H % 16 == 0 and W % 16 == 0 and frame.dtype == np.uint8
    rgb = frame[..., ::-1] if channel_order == 'bgr' else frame
    y, cb, cr = rgb_to_ycc(rgb)
    ql, qc = quality_tables(quality)
    out = []
    for plane, q in ((y, ql), (downsample_h2v2(cb), qc), (downsample_h2v2(cr), qc)):
        c = fdct_islow(_blocks(plane - 128), track)
        out.append(quantise(c.reshape(c.shape[:2] + (64,)), q).astype(np.int16))
    return ql, qc, out


def record_from(width, height, h, v, quants, coef):
    """the record bytes (uint8) dir_jpeg_decode_coefficients writes: header (include/dir_jpeg.h) + coefficients"""
    nc = len(coef)
    hdr = np.zeros(HEADER_BYTES, np.uint8)
    i32 = hdr[:96].view(np.int32)
    hm, vm = max(h), max(v)
    mcux, mcuy = -(-width // (8 * hm)), -(-height // (8 * vm))
    i32[0:8] = (MAGIC, width, height, nc, hm, vm, mcux, mcuy)
    off = 0
    for c in range(nc):
        i32[8 + c], i32[11 + c] = h[c], v[c]
        i32[14 + c], i32[17 + c] = mcux * h[c], mcuy * v[c]
        assert coef[c].shape == (mcuy * v[c], mcux * h[c], 64)
        i32[20 + c] = off
        off += coef[c].size
        hdr[96 + 128 * c:96 + 128 * (c + 1)].view(np.uint16)[:] = quants[c]
    i32[23] = off
    return np.concatenate([hdr] + [np.ascontiguousarray(c, np.int16).reshape(-1).view(np.uint8) for c in coef])


def encode_record(frame, quality, channel_order='bgr', track=None):
    """what dir_jpeg_encode_records writes for one frame"""
    ql, qc, coef = coefficients(frame, quality, channel_order, track)
    return record_from(frame.shape[1], frame.shape[0], (2, 1, 1), (2, 1, 1), (ql, qc, qc), coef)


def _ehuff(counts, symbols):
    out, code, k = {}, 0, 0
    for ln in range(1, 17):
        for _ in range(counts[ln - 1]):
            out[symbols[k]] = (code, ln)
            code += 1
            k += 1
        code <<= 1
    return out


def _segment(marker, payload):
    return bytes([0xFF, marker, (len(payload) + 2) >> 8, (len(payload) + 2) & 255]) + bytes(payload)


def file_from(width, height, h, v, quants, coef):
    """the baseline JFIF file of include/dir_jpeg_enc.h from per-component coefficient arrays [blocks_y, blocks_x, 64]"""
    nc = len(coef)
    tq = [0, 1, 1 if nc < 3 or np.array_equal(quants[2], quants[1]) else 2][:nc]
    out = bytearray(b'\xff\xd8') + _segment(0xE0, b'JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00')
    for t in range(max(tq) + 1):
        out += _segment(0xDB, bytes([t]) + bytes(int(quants[t][z]) for z in J.ZIGZAG))
    sof = [8, height >> 8, height & 255, width >> 8, width & 255, nc]
    for c in range(nc):
        sof += [c + 1, (h[c] << 4) | v[c], tq[c]]
    out += _segment(0xC0, sof)
    tabs = [(0x00, DC_LUMA), (0x10, AC_LUMA)] + ([(0x01, DC_CHROMA), (0x11, AC_CHROMA)] if nc == 3 else [])
    for tid, (counts, syms) in tabs:
        out += _segment(0xC4, [tid] + counts + syms)
    sos = [nc]
    for c in range(nc):
        sos += [c + 1, 0x11 if c else 0x00]
    out += _segment(0xDA, sos + [0, 63, 0])
    dc = [_ehuff(*DC_LUMA), _ehuff(*DC_CHROMA)]
    ac = [_ehuff(*AC_LUMA), _ehuff(*AC_CHROMA)]
    acc, n, pred = 0, 0, [0] * nc
    scan = bytearray()

    def put(code, size):
        nonlocal acc, n
        acc = (acc << size) | code
        n += size
        while n >= 8:
            byte = (acc >> (n - 8)) & 255
            scan.append(byte)
            if byte == 255:
                scan.append(0)
            n -= 8
        acc &= (1 << n) - 1
    hm, vm = max(h), max(v)
    mcux, mcuy = -(-width // (8 * hm)), -(-height // (8 * vm))
    for my in range(mcuy):
        for mx in range(mcux):
            for c in range(nc):
                for by in range(v[c]):
                    for bx in range(h[c]):
                        blk = [int(x) for x in coef[c][my * v[c] + by, mx * h[c] + bx][J.ZIGZAG]]
                        d = blk[0] - pred[c]
                        pred[c] = blk[0]
                        nb = abs(d).bit_length()
                        assert nb <= 11
                        put(*dc[min(c, 1)][nb])
                        if nb:
                            put((d - 1 if d < 0 else d) & ((1 << nb) - 1), nb)
                        run = 0
                        for k in range(1, 64):
                            x = blk[k]
                            if x == 0:
                                run += 1
                                continue
                            while run > 15:
                                put(*ac[min(c, 1)][0xF0])
                                run -= 16
                            nb = abs(x).bit_length()
                            assert nb <= 10
                            put(*ac[min(c, 1)][(run << 4) | nb])
                            put((x - 1 if x < 0 else x) & ((1 << nb) - 1), nb)
                            run = 0
                        if run:
                            put(*ac[min(c, 1)][0])
    if n:
        put((1 << (8 - n)) - 1, 8 - n)
    return bytes(out + scan + b'\xff\xd9')


def encode_file(frame, quality, channel_order='bgr'):
    """uint8 [H, W, 3] -> the bytes Image.fromarray(rgb).save(format='JPEG', quality=quality, subsampling=2) writes"""
    ql, qc, coef = coefficients(frame, quality, channel_order)
    return file_from(frame.shape[1], frame.shape[0], (2, 1, 1), (2, 1, 1), (ql, qc, qc), coef)
