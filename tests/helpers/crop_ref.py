"""float64 numpy restatement of the crop rules of csrc/crop.hip (include/dir_hip.h, "hand crops from full frames"): cut_img's matrix
(dataset/dataset_utils.py:26-58), the chain from one stage of the network's output to the next frame's matrix, and the way from crop
coordinates back to frame pixels.  Written independently of the kernels; every operation is one IEEE double operation, in the reference's
order, so equality with the kernels and with the reference's own matrices (tests/golden/g25_crop.npz) is to the bit.  The pixel rule is
tests/helpers/augment_ref.py::warp_affine_u8."""
import numpy as np

MIN_SCALE, MAX_SCALE, MAX_COORD = 2.0 ** -6, 2.0 ** 6, 2.0 ** 20
LABEL_STEP = 32          # G25 keeps every 32nd transformed label


def matrix_from_extremes(Min, Max, ratio=0.8, size=256):
    """Min, Max: the per-axis extremes (x, y) -> (M float64 [2,3], valid).  Invalid: M is zeros."""
    Min, Max = np.asarray(Min, np.float64), np.asarray(Max, np.float64)
    zero = np.zeros((2, 3))
    if not (np.isfinite(Min).all() and np.isfinite(Max).all()):
        return zero, 0
    mid = (Min + Max) / 2
    with np.errstate(all='ignore'):
        L = np.max(Max - Min) / 2 / np.float64(ratio)
        if not (np.isfinite(L) and L > 0):
            return zero, 0
        s = np.float64(size / 2) / L
    if not MIN_SCALE <= s <= MAX_SCALE:
        return zero, 0
    if max(abs(mid[0] - L), abs(mid[0] + L), abs(mid[1] - L), abs(mid[1] + L)) > MAX_COORD:
        return zero, 0
    return np.array([[s, 0.0, s * (L - mid[0])], [0.0, s, s * (L - mid[1])]]), 1


def matrix_from_points(point_sets, ratio=0.8, size=256):
    """cut_img's matrix for a list of [N,2] point sets (converted to double first)"""
    pts = [np.asarray(p, np.float64) for p in point_sets]
    if not all(np.isfinite(p).all() for p in pts):
        return np.zeros((2, 3)), 0
    return matrix_from_extremes(np.min([p.min(0) for p in pts], 0), np.max([p.max(0) for p in pts], 0), ratio, size)


def matrix_from_box(box, ratio=0.8, size=256):
    """a tight box (x0, y0, x1, y1), float32 as the kernel receives it: its two corners are the point set"""
    b = np.asarray(box, np.float32).astype(np.float64)
    return matrix_from_points([b.reshape(2, 2)], ratio, size)


def frame_points(mesh, proj, M_prev, size=256):
    """one hand of one stage: mesh float32 [778,3], proj float32 [3] = (s, tx, ty), M_prev [2,3] -> frame positions float64 [778,2]:
    uv = s xy + t in float32 (multiply, then add), crop position (uv + 1) size / 2 in double, then back through M_prev"""
    mesh, proj, M_prev = np.asarray(mesh, np.float32), np.asarray(proj, np.float32), np.asarray(M_prev, np.float64).reshape(2, 3)
    with np.errstate(all='ignore'):
        uv = (proj[0] * mesh[:, :2]).astype(np.float32) + proj[1:3]
        c = (uv.astype(np.float64) + 1.0) * np.float64(size) / 2.0
        return (c - M_prev[:, 2]) / M_prev[0, 0]


def matrix_from_meshes(mesh_left, mesh_right, proj_left, proj_right, M_prev, ratio=0.8, size=256):
    """-> (M_next [2,3], valid); an invalid result holds M_prev"""
    M_prev = np.asarray(M_prev, np.float64).reshape(2, 3)
    M, ok = matrix_from_points([frame_points(mesh_left, proj_left, M_prev, size), frame_points(mesh_right, proj_right, M_prev, size)], ratio, size)
    return (M, 1) if ok else (M_prev.copy(), 0)


def to_frame_pixels(uv, M, size=256):
    """normalised crop coordinates uv [N,2] in -1..1 -> frame pixels, float64: ((uv + 1) size / 2 - M[:, 2]) / M[0, 0]"""
    M = np.asarray(M, np.float64).reshape(2, 3)
    return ((np.asarray(uv).astype(np.float64) + 1.0) * np.float64(size) / 2.0 - M[:, 2]) / M[0, 0]


def frame_camera(proj, M, size=256):
    """(s, tx, ty) of uv = s xy + t -> (scale_px, trans_px [2]) float64 with frame pixel = scale_px xy + trans_px"""
    proj, M = np.asarray(proj).astype(np.float64), np.asarray(M, np.float64).reshape(2, 3)
    return proj[0] * np.float64(size) / 2.0 / M[0, 0], ((proj[1:3] + 1.0) * np.float64(size) / 2.0 - M[:, 2]) / M[0, 0]


def transform_labels(label2d, M):
    """cut_img's label2d_list_out for one float64 set [N,2]: [x, y, 1] @ M.T, the three products summed left to right"""
    p, M = np.asarray(label2d, np.float64), np.asarray(M, np.float64).reshape(2, 3)
    return np.stack([p[:, 0] * M[r, 0] + p[:, 1] * M[r, 1] + 1.0 * M[r, 2] for r in range(2)], 1)


def transform_camera(K, M):
    """cut_img's update of a float64 3x3 intrinsic matrix"""
    K, M = np.array(K, np.float64), np.asarray(M, np.float64).reshape(2, 3)
    K[0, 0] = K[0, 0] * M[0, 0]
    K[1, 1] = K[1, 1] * M[1, 1]
    K[0, 2] = K[0, 2] * M[0, 0] + M[0, 2]
    K[1, 2] = K[1, 2] * M[1, 1] + M[1, 2]
    return K


def make_case(seed):
    """the seeded inputs of one G25 case: two float64 point sets [778,2] around a frame position, and a float64 3x3 intrinsic matrix"""
    rng = np.random.RandomState(seed)
    centre = rng.uniform(100, 900, 2)
    spread = rng.uniform(20, 160)
    pts = [centre + rng.uniform(-40, 40, 2) + rng.normal(0, spread / 3, (778, 2)) for _ in range(2)]
    K = np.array([[rng.uniform(1000, 2000), 0, rng.uniform(200, 600)], [0, rng.uniform(1000, 2000), rng.uniform(200, 600)], [0, 0, 1.0]])
    return pts, K


def checksum(pts, K):
    return np.float64(sum(float(np.asarray(p, np.float64).sum()) for p in pts) + float(K.sum()))
