"""numpy restatement of the anti-aliased crop of csrc/crop.hip (include/dir_hip.h, "anti-aliased crops"): for a matrix that shrinks the
frame without rotating, shearing or mirroring it, Pillow's Image.resize(size, BILINEAR, box) -- a triangle filter as wide as the shrink,
coefficients normalised in float64 and rounded to 22 fractional bits, horizontal pass then vertical pass with a uint8 between them
(libImaging/Resample.c: precompute_coeffs, normalize_coeffs_8bpc, ImagingResampleHorizontal_8bpc / Vertical_8bpc) -- on the frame-pixel
box the matrix cuts out, WITHOUT Pillow's clamping of the window to the image: a tap outside the frame reads 0 and keeps its weight, the
zero border of the plain crop.  Every other matrix: tests/helpers/augment_ref.py::warp_affine_u8.  Every coefficient operation is one
IEEE double operation in the order written in the header; the pixel sums are integers.  Written independently of the kernel."""
import math

import numpy as np
from augment_ref import warp_affine_u8

PRECISION_BITS = 22
MIN_SCALE = 2.0 ** -6


def is_shrinking(M):
    """the matrices that get the anti-aliased rule: axis-aligned, not mirrored, and smaller than 1 along at least one axis"""
    m = np.asarray(M, np.float64).reshape(6)
    return bool(m[1] == 0 and m[3] == 0 and m[0] > 0 and m[4] > 0 and min(m[0], m[4]) < 1)


def box_from_matrix(M, size):
    """-> (x0, y0, x1, y1): the frame-pixel edges of the crop in Pillow's terms (pixel k covers [k, k + 1)); per axis
    in0 = 0.5 - (t + 0.5) / s, in1 = in0 + size / s"""
    m = np.asarray(M, np.float64).reshape(6)
    box = []
    for s, t in ((float(m[0]), float(m[2])), (float(m[4]), float(m[5]))):
        in0 = 0.5 - (t + 0.5) / s
        box.append((in0, in0 + float(size) / s))
    return (box[0][0], box[1][0], box[0][1], box[1][1])


def coefficients(in0, in1, size):
    """one axis -> per output position (first tap, [K]): the taps first tap .. first tap + len(K) - 1 and their 22-bit weights"""
    in0, in1 = float(in0), float(in1)
    scale = (in1 - in0) / float(size)
    fs = max(scale, 1.0)
    support = fs
    out = []
    for u in range(size):
        c = in0 + (float(u) + 0.5) * scale
        xmin, xmax = int(math.floor(c - support + 0.5)), int(math.floor(c + support + 0.5))
        k, ww = [], 0.0
        for x in range(xmin, xmax):
            w = max(0.0, 1.0 - abs((float(x) - c + 0.5) / fs))
            k.append(w)
            ww += w                                                     # in tap order: a double sum is not order-free
        out.append((xmin, [int(w / ww * float(1 << PRECISION_BITS) + 0.5) for w in k]))
    return out


def _pass(src, coeffs):
    """src int64 [N, L, C], filtered along axis 1 -> uint8-valued int64 [N, len(coeffs), C]; a tap outside 0 .. L - 1 adds nothing"""
    n = src.shape[1]
    out = np.zeros((src.shape[0], len(coeffs), src.shape[2]), np.int64)
    for u, (xmin, K) in enumerate(coeffs):
        acc = np.full((src.shape[0], src.shape[2]), 1 << (PRECISION_BITS - 1), np.int64)
        for j, kk in enumerate(K):
            if 0 <= xmin + j < n:
                acc += kk * src[:, xmin + j]
        out[:, u] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def resample_box(frame, box, size):
    """frame uint8 [H,W,C], box (x0, y0, x1, y1) in frame pixels -> uint8 [size,size,C]: horizontal pass, rounded to uint8, then the
    vertical pass over it"""
    src = np.asarray(frame).astype(np.int64)
    tmp = _pass(src, coefficients(box[0], box[2], size))                                  # [H, size, C]
    out = _pass(tmp.transpose(1, 0, 2), coefficients(box[1], box[3], size))               # [size(x), size(y), C]
    return out.transpose(1, 0, 2).astype(np.uint8)


def crop_area(frame, M, size):
    """the crop with antialias on -> uint8 [size,size,C]: the anti-aliased rule where is_shrinking(M), the plain warp elsewhere"""
    if is_shrinking(M):
        m = np.asarray(M, np.float64).reshape(6)
        assert min(m[0], m[4]) >= MIN_SCALE, 'a scale below 2^-6 is refused (DIR_CROP_BAD_MATRIX), not cropped'
        return resample_box(frame, box_from_matrix(M, size), size)
    return warp_affine_u8(frame, M, (size, size))
