"""Writes tests/golden/g26_jpeg_enc.npz: small frames with the exact bytes Pillow's libjpeg-turbo wrote for them and the pixels it decodes
from those bytes -- the pin of the JPEG encode path (tests/helpers/jpeg_enc_ref.py, csrc/jpeg_enc_huff.c, csrc/jpeg_enc.hip).

    python tools/gen_jpeg_enc_golden.py            (needs Pillow; the tests only read the file)

Per case NAME:  NAME.frame  uint8 [H,W,3] in the project's frame convention (BGR, what cv.imwrite receives)
                NAME.q      the quality
                NAME.jpg    the bytes of Image.fromarray(frame[..., ::-1]).save(format='JPEG', quality=q, subsampling=2)
                NAME.pix    Pillow's decode of those bytes, BGR (what cv.imread / dataset.decode_bgr return)
H and W are multiples of 16 (whole MCUs), 4:2:0: the scope of dir_jpeg_encode_records."""
import io
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'tests', 'golden', 'g26_jpeg_enc.npz')


def checker(h, w, period, phases):
    yy, xx = np.mgrid[0:h, 0:w]
    return np.stack([((((yy + p) // period) + ((xx + 2 * p) // period)) & 1) * 255 for p in phases], -1).astype(np.uint8)


def rendered_like(size=256):
    """black background, two blobs with hard edges and smooth colour inside: the look of the dense/ frames"""
    yy, xx = np.mgrid[0:size, 0:size].astype(np.float64)
    img = np.zeros((size, size, 3), np.float64)
    for cx, cy, rx, ry, ph in ((90, 120, 55, 80, 0.0), (170, 140, 50, 70, 1.7)):
        inside = ((xx - cx) / rx) ** 2 + ((yy - cy) / ry) ** 2 < 1 + 0.15 * np.sin(xx / 6.0 + ph) * np.cos(yy / 5.0)
        col = np.stack([127 + 120 * np.sin(xx / 23.0 + ph + c) * np.cos(yy / 31.0 - c) for c in range(3)], -1)
        img[inside] = col[inside]
    return np.clip(img, 0, 255).astype(np.uint8)


def cases():
    rng = np.random.RandomState(26)
    out = []
    for h, w, q in ((16, 16, 75), (32, 48, 95), (48, 32, 50)):
        out.append(('noise_%dx%d_q%d' % (h, w, q), rng.randint(0, 256, (h, w, 3)).astype(np.uint8), q))
    for period in (1, 8):
        for q in (100, 1):
            out.append(('checker_p%d_q%d' % (period, q), checker(32, 32, period, (0, 1, 3) if period == 1 else (0, 4, 8)), q))
    for name, bgr in (('zero', (0, 0, 0)), ('white', (255, 255, 255)), ('blue', (255, 0, 0)), ('green', (0, 255, 0)), ('red', (0, 0, 255)),
                      ('yellow', (0, 255, 255))):
        out.append(('const_%s_q95' % name, np.tile(np.array(bgr, np.uint8), (16, 16, 1)), 95))
    flat = np.full((48, 64, 3), 30, np.uint8)
    flat[5:29, 9:40] = (200, 40, 90)
    flat[20:44, 30:61] = (10, 220, 160)
    flat[0:7, 50:64] = (255, 255, 0)
    out.append(('rects_q30', flat, 30))
    out.append(('rendered_256_q95', rendered_like(), 95))
    return out


def main():
    from PIL import Image
    data = {}
    for name, frame, q in cases():
        buf = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(frame[..., ::-1])).save(buf, format='JPEG', quality=q, subsampling=2)
        pix = np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert('RGB'))[..., ::-1]
        data[name + '.frame'] = frame
        data[name + '.q'] = np.int32(q)
        data[name + '.jpg'] = np.frombuffer(buf.getvalue(), np.uint8)
        data[name + '.pix'] = np.ascontiguousarray(pix)
    np.savez_compressed(OUT, **data)
    print('%s: %d cases, %d bytes' % (OUT, len(data) // 4, os.path.getsize(OUT)))


if __name__ == '__main__':
    main()
