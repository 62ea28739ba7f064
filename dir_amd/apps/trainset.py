"""Training input (SURVEY.md 8f rank 2's data side): dataset/interhand.py:__getitem__ of the 'train' split for whole batches on the GPU.

  sample_params     get_aug_config (utils/utils.py:463-473), the motion-blur draw (:526-533) and add_noise's a, b (:446-452), per sample,
                    in the reference's order and ranges, from a seeded numpy Generator; plus the float32 2x3 matrix of get_affine_mat
                    (:300-312) and the float32 motion-blur kernel (cv.getRotationMatrix2D + the float cv.warpAffine of :531, restated below)
  augment_batch     uint8 img / mask / dense frames + GT -> the reference's (inputs, targets, meta_info) dicts, three launches
                    (dir_train_augment_images: blur pre-pass + image pass; dir_train_augment_labels)
  TrainBatches      DataLoader(InterHandDataset(data_path, 'train'), shuffle=True, drop_last=True) of train.py:64-70: DecodeRing carries
                    img / mask / dense (or img only, with dense_color: mask / dense rendered from gt_batch's meshes by
                    dir_amd.utils.vis_utils), gt_batch runs the GT MANO, augment_batch the rest

Matching the reference's random STREAM is not a goal (its DataLoader workers seed themselves); the distributions are the reference's.  The
Gaussian term of add_noise comes from a counter RNG on the GPU (dir_train_noise_field, include/dir_hip.h), float32 instead of float64 draws.
Parity: the label maths is pinned to the reference's own functions (tests/golden/g23_train_aug.npz); the image pass is bit-exact with a
numpy restatement of the published OpenCV warpAffine / filter2D rules (tests/helpers/augment_ref.py), unpinned against the library, which
is not installed where this was written.
"""
import ctypes as C
import math

import numpy as np
import torch

from .. import _capi

IMG_SIZE = 256
MAX_BLUR = 9
MEAN = (0.485, 0.456, 0.406)            # dataset/interhand.py:108-109
STD = (0.229, 0.224, 0.225)

# dir_aug_params (include/dir_hip.h), 400 bytes
AUG_DTYPE = np.dtype([('M', '<f4', (6,)), ('flip', '<i4'), ('blur', '<i4'), ('a', '<f8', (3,)), ('b', '<f8'),
                      ('kernel', '<f4', (MAX_BLUR * MAX_BLUR,)), ('pad_', '<f4', (3,))], align=True)
assert AUG_DTYPE.itemsize == 400


def affine_mat(theta, scale, u, v, size=IMG_SIZE):
    """utils.py:300-312 get_affine_mat(theta, scale, u, v, size, size): the same float32 numpy operations -> float32 [3,3]"""
    center = np.array([size / 2, size / 2, 1], dtype='float32')
    t = np.deg2rad(theta)
    rot = np.zeros((3, 3), dtype='float32')
    rot[0, 0], rot[0, 1], rot[1, 0], rot[1, 1], rot[2, 2] = math.cos(t), -math.sin(t), math.sin(t), math.cos(t), 1.0
    tr = np.matmul((np.identity(3, dtype='float32') - rot), center)
    rot[0, 2], rot[1, 2] = tr[0], tr[1]
    sc = np.zeros((3, 3), dtype='float32')
    sc[0, 0], sc[1, 1], sc[2, 2] = scale, scale, 1.0
    ts = np.matmul((np.identity(3, dtype='float32') - sc), center)
    sc[0, 2], sc[1, 2] = ts[0], ts[1]
    trans = np.identity(3, dtype='float32')
    trans[0, 2], trans[1, 2] = u, v
    return np.matmul(trans, np.matmul(sc, rot))


def warp_coords(M, dw, dh):
    """cv.warpAffine's source coordinates (INTER_LINEAR): M (2x3, forward) inverted in double, per row / column 10-bit fixed point
    (round half to even), summed, rounded to 5 bits.  -> integer (sx, sy) and 5-bit fractions (fx, fy), int64 [dh, dw]"""
    M = np.asarray(M, np.float64).reshape(6)
    D = M[0] * M[4] - M[1] * M[3]
    D = 1. / D if D != 0 else 0.
    m0, m1, m3, m4 = M[4] * D, M[1] * -D, M[3] * -D, M[0] * D
    m2, m5 = -m0 * M[2] - m1 * M[5], -m3 * M[2] - m4 * M[5]
    x, y = np.arange(dw, dtype=np.float64), np.arange(dh, dtype=np.float64)
    X0 = np.rint((m1 * y + m2) * 1024).astype(np.int64) + 16
    Y0 = np.rint((m4 * y + m5) * 1024).astype(np.int64) + 16
    X = (X0[:, None] + np.rint(m0 * x * 1024).astype(np.int64)[None, :]) >> 5
    Y = (Y0[:, None] + np.rint(m3 * x * 1024).astype(np.int64)[None, :]) >> 5
    return X >> 5, Y >> 5, X & 31, Y & 31


def warp_f32(src, M, dsize):
    """cv.warpAffine(src, M, dsize) for a float32 single-channel image (INTER_LINEAR, BORDER_CONSTANT 0): the fixed-point coordinates of
    warp_coords, float32 weights (1 - f, f) with f = k / 32, taps outside the image read 0, t = s00 w0 + s01 w1 + s10 w2 + s11 w3 in float32"""
    src = np.asarray(src, np.float32)
    h, w = src.shape
    sx, sy, fx, fy = warp_coords(M, dsize[0], dsize[1])
    wx1, wy1 = fx.astype(np.float32) * np.float32(1 / 32), fy.astype(np.float32) * np.float32(1 / 32)
    wx0, wy0 = np.float32(1) - wx1, np.float32(1) - wy1

    def tap(dx, dy):
        xx, yy = sx + dx, sy + dy
        ok = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
        return np.where(ok, src[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)], np.float32(0))
    return tap(0, 0) * (wy0 * wx0) + tap(1, 0) * (wy0 * wx1) + tap(0, 1) * (wy1 * wx0) + tap(1, 1) * (wy1 * wx1)


def motion_blur_kernel(size, angle):
    """utils.py:526-533's kernel: a horizontal line through the middle row, rotated by cv.getRotationMatrix2D(centre, angle, 1) -- `angle` is
    the radians value the reference passes where degrees are expected, kept -- normalised to sum 1.  float32 [size, size]"""
    k = np.zeros((size, size), dtype=np.float32)
    k[(size - 1) // 2, :] = np.ones(size, dtype=np.float32)
    c = float(np.float32(size / 2 - 0.5))                                  # Point2f centre
    ang = angle * math.pi / 180                                            # getRotationMatrix2D: degrees -> radians, in double
    alpha, beta = math.cos(ang), math.sin(ang)
    M = np.array([[alpha, beta, (1 - alpha) * c - beta * c], [-beta, alpha, beta * c + (1 - alpha) * c]])
    k = warp_f32(k, M, (size, size))
    return k * (1.0 / np.sum(k))


def sample_params(rng, n, augment=True, size=IMG_SIZE):
    """per-sample augmentation draws of dataset/interhand.py:__getitem__ -> numpy dir_aug_params [n].  augment=True (split 'train'):
    get_aug_config(0.1, 180, 10, True) -- scale 1 +- 0.1, rot +-180 deg, tx / ty +-10 px, flip p = 0.5 --, blur p = 0.3 (size randint(3, 10),
    angle uniform(-180, 180) * pi / 180), then add_noise's a ~ U(0.7, 1.3)^3 and b = 255 * 0.05 * (2u - 1).  augment=False (val / test):
    identity warp, no flip, no blur, the noise draws only (the reference applies add_noise to every split)."""
    P = np.zeros(n, AUG_DTYPE)
    ident = np.array([1, 0, 0, 0, 1, 0], np.float32)
    for i in range(n):
        if augment:
            scale = 1 + (rng.random() * 2 - 1) * 0.1
            rot = (rng.random() * 2 - 1) * 180
            tx = (rng.random() * 2 - 1) * 10
            ty = (rng.random() * 2 - 1) * 10
            P['flip'][i] = rng.random() <= 0.5
            P['M'][i] = affine_mat(rot, scale, tx, ty, size)[:2].reshape(6)
            if rng.random() <= 0.3:
                ks = int(rng.integers(3, 10))
                P['blur'][i] = ks
                P['kernel'][i, :ks * ks] = motion_blur_kernel(ks, rng.uniform(-180, 180) * np.pi / 180).reshape(-1)
        else:
            P['M'][i] = ident
        P['a'][i] = rng.uniform(1 - 0.3, 1 + 0.3, 3)
        P['b'][i] = 255.0 * 0.05 * (2 * rng.random() - 1)
    return P


def params_to_device(params, device):
    """numpy dir_aug_params [n] -> uint8 device tensor [n, 400] (what the entry points read)"""
    assert params.dtype == AUG_DTYPE
    return torch.from_numpy(np.ascontiguousarray(params).view(np.uint8).reshape(len(params), AUG_DTYPE.itemsize)).to(device, non_blocking=True)


def _nm():
    return (C.c_float * 3)(*MEAN), (C.c_float * 3)(*STD)


def noise_field(seed, B, device='cuda'):
    """the Gaussian term of add_noise that augment_batch generates for `seed` (dir_train_noise_field): float32 [B,256,256,3]"""
    out = torch.empty(B, IMG_SIZE, IMG_SIZE, 3, dtype=torch.float32, device=device)
    with torch.cuda.device(out.device):
        _capi.check(_capi.lib().dir_train_noise_field(C.c_ulonglong(int(seed) & (2 ** 64 - 1)), _capi.ptr(out), B, _capi.stream_ptr()),
                    'dir_train_noise_field')
    return out


_LABEL_KEYS = ('joint_2d_left', 'mesh_2d_left', 'joint_2d_right', 'mesh_2d_right', 'joint_3d_left', 'mesh_3d_left', 'joint_3d_right',
               'mesh_3d_right')


def augment_batch(frames, masks, dense, annos, params, noise=None, mano_layer=None, seed=0, augment=True, scratch=None):
    """dataset/interhand.py:__getitem__ after the file reads, for a batch, on the GPU.
    frames / masks / dense: uint8 cuda [B,256,256,3] BGR; annos: float32 cuda [B,155] (InterHandSplit.anno layout; needs `mano_layer`, the
    GT layers) or the tuple gt_batch returned; params: numpy dir_aug_params [B] (sample_params) or their uint8 device copy [B,400];
    noise: float32 cuda [B,256,256,3] (255 * N(0, 0.01)) or None = generated from `seed`; augment=False: the labels pass through
    (the val / test splits).  Returns (inputs, targets, meta_info) as the reference's dicts with a batch dimension."""
    from .dataset import gt_batch
    _capi.require_cuda(frames, masks, dense)
    B, dev = frames.shape[0], frames.device
    for t in (frames, masks, dense):
        assert t.dtype == torch.uint8 and t.is_contiguous() and tuple(t.shape) == (B, IMG_SIZE, IMG_SIZE, 3), 'augment_batch: frames must be uint8 [B,256,256,3]'
    if isinstance(params, np.ndarray):
        assert len(params) == B
        params = params_to_device(params, dev)
    assert params.dtype == torch.uint8 and tuple(params.shape) == (B, AUG_DTYPE.itemsize) and params.is_contiguous()
    if noise is not None:
        assert noise.dtype == torch.float32 and noise.is_contiguous() and tuple(noise.shape) == (B, IMG_SIZE, IMG_SIZE, 3)
    gt = tuple(annos) if isinstance(annos, (tuple, list)) else gt_batch(mano_layer, annos)
    jl, vl, jr, vr, j2l, v2l, j2r, v2r, K = [g.contiguous().float() for g in gt]
    f32 = dict(dtype=torch.float32, device=dev)
    inputs = {'img': torch.empty(B, 3, IMG_SIZE, IMG_SIZE, **f32), 'img_rgb': torch.empty(B, IMG_SIZE, IMG_SIZE, 3, **f32),
              'mask_rgb': torch.empty(B, IMG_SIZE, IMG_SIZE, 3, **f32)}
    targets = {'seg': torch.empty(B, 1, IMG_SIZE, IMG_SIZE, **f32), 'dense': torch.empty(B, 3, IMG_SIZE, IMG_SIZE, **f32)}
    for k in _LABEL_KEYS:
        targets[k] = torch.empty(B, 21 if k.startswith('joint') else 778, 3, **f32)
    meta_info = {'camera': K, 'center_left': torch.empty(B, 1, 3, **f32), 'center_right': torch.empty(B, 1, 3, **f32)}
    if scratch is None:
        scratch = torch.empty(B, IMG_SIZE, IMG_SIZE, 3, dtype=torch.uint8, device=dev)
    mean, std = _nm()
    L = _capi.lib()
    P = _capi.ptr
    with torch.cuda.device(dev):
        _capi.check(L.dir_train_augment_images(P(params), P(frames), P(masks), P(dense), P(noise) if noise is not None else None,
                                               C.c_ulonglong(int(seed) & (2 ** 64 - 1)), mean, std, P(scratch), P(inputs['img']),
                                               P(inputs['img_rgb']), P(inputs['mask_rgb']), P(targets['seg']), P(targets['dense']), B,
                                               _capi.stream_ptr()), 'dir_train_augment_images')
        ins = (C.c_void_p * 8)(*[P(t) for t in (jl, vl, jr, vr, j2l, v2l, j2r, v2r)])
        outs = (C.c_void_p * 10)(*[P(targets[k]) for k in _LABEL_KEYS] + [P(meta_info['center_left']), P(meta_info['center_right'])])
        _capi.check(L.dir_train_augment_labels(P(params) if augment else None, C.byref(ins), P(K), C.byref(outs), B, _capi.stream_ptr()),
                    'dir_train_augment_labels')
    return inputs, targets, meta_info


class TrainBatches(object):
    """train.py:64-70's loader: batches of the prepared split, shuffled per epoch, drop_last, as the reference's three dicts on the device.

        batches = TrainBatches(data_path, mano_layer, 'train', batch_size=32, workers=8, seed=0)
        for epoch in range(n):
            for inputs, targets, meta_info in batches:          # a new permutation per pass
                loss = train_step(params, buffers, inputs['img'], targets, meta_info, faces, optimizer)

    mano_layer: the GT MANO layers ({'left', 'right'}, dataset.gt_layers_from_checkpoint).  augment=False (val / test): no flip, blur or
    warp, but the noise is applied, as the reference does.  Decode: `workers` processes of a DecodeRing carry img / mask / dense
    (records=True: the Huffman decode only, the rest of the JPEG decode on the GPU).  The parameter draws of every batch are kept in
    `self.last_params` (numpy dir_aug_params) and the noise seed in `self.last_seed`.

    dense_color: the dense colour table (the [778,3] array in 0..1 of get_dense_color_path(), or the pickle's path).  Given, mask and
    dense are not read from files: they are rendered per batch (csrc/render.hip, render_data's rules) from the camera-frame vertices of
    gt_batch, whose tuple augment_batch then reuses, so the ground-truth MANO runs once; only img/ is decoded.  These frames are the
    arrays cv.imwrite would receive.  With jpeg_round_trip=False (the default) they go to augment_batch as they are, without the JPEG
    round trip the files have been through, so they are not the file path's bytes.  With jpeg_round_trip=True they pass through the JPEG
    encode and decode at quality 95 on the device first (dir_amd.apps.jpeg.RoundTrip: dir_jpeg_encode_records, then
    dir_jpeg_decode_records), and are then exactly what the file path decodes from the mask/ and dense/ files render_split writes.
    The faces are the right GT layer's (ManoLayer.get_faces()); a layer without faces (a checkpoint without th_faces) is an error.

    shuffle=False: every pass reads the split in file order (the reference's test loader, train.py:215-220; drop_last as well) and draws
    no permutation.  `self.last_perm` holds the file indices of the pass that was started last, in the order they are read."""

    def __init__(self, data_path, mano_layer, split='train', batch_size=32, workers=8, seed=0, augment=True, records=True, device='cuda',
                 dense_color=None, shuffle=True, jpeg_round_trip=False):
        from .dataset import InterHandSplit
        self.data_path, self.split, self.mano_layer = data_path, split, mano_layer
        self.bs, self.workers, self.augment, self.records = batch_size, workers, augment, records
        self.device = torch.device(device)
        self.rng = np.random.default_rng(seed)
        self.seed, self.shuffle, self.last_perm = seed, bool(shuffle), None
        self.n = len(InterHandSplit(data_path, split))
        self.epoch = 0
        self.last_params, self.last_seed = None, None
        self.render = self.round_trip = None
        if jpeg_round_trip and dense_color is None:
            raise ValueError('TrainBatches: jpeg_round_trip applies to rendered targets (dense_color=...)')
        if dense_color is not None:
            from ..utils import vis_utils as V
            self.render = (torch.from_numpy(V.faces_from_layers(mano_layer)).to(self.device),
                           torch.from_numpy(V.load_dense_colors(dense_color)).to(self.device),
                           torch.empty(int(_capi.lib().dir_render_workspace_bytes(batch_size)), dtype=torch.uint8, device=self.device))
            if jpeg_round_trip:
                from .jpeg import RoundTrip
                self.round_trip = RoundTrip(batch_size, IMG_SIZE, quality=95, channel_order='bgr', device=self.device)

    def __len__(self):
        return self.n // self.bs

    def __iter__(self):
        from .dataset import IMG_SIZE as S, DecodeRing
        perm = (self.rng.permutation(self.n) if self.shuffle else np.arange(self.n))[:len(self) * self.bs]
        self.last_perm = perm
        self.epoch += 1
        if len(perm) == 0:
            return
        nf = 1 if self.render is not None else 3                          # frames decoded per sample: img (+ mask, dense)
        ring = DecodeRing(self.data_path, self.split, self.bs, workers=self.workers, indices=perm.tolist(), records=self.records,
                          extra=('mask', 'dense') if nf == 3 else ())
        dev, bs = self.device, self.bs
        copy_stream = torch.cuda.Stream(dev)
        dec = None
        if self.records:
            from .jpeg import RecordDecoder
            dec = RecordDecoder(nf * bs, ring.record_bytes, S, dev)
        try:
            for item in ring:
                frames, annos = item[0], item[1]
                params = sample_params(self.rng, bs, self.augment)
                seed = int(self.rng.integers(0, 2 ** 63))
                main = torch.cuda.current_stream(dev)
                with torch.cuda.stream(copy_stream):
                    host = [frames] + (list(item[3]) if nf == 3 else [])
                    raw = torch.empty((nf * bs,) + tuple(frames.shape[1:]), dtype=torch.uint8, device=dev)
                    for j, h in enumerate(host):
                        raw[j * bs:(j + 1) * bs].copy_(h, non_blocking=True)
                    an = annos.to(dev, non_blocking=True)
                    pr = params_to_device(params, dev)
                    copied = torch.cuda.Event()
                    copied.record()
                copied.synchronize()                                       # the ring's buffers may go back to the decoders
                main.wait_stream(copy_stream)
                for t in (raw, an, pr):
                    t.record_stream(main)
                if dec is not None:
                    fr = torch.empty(nf * bs, S, S, 3, dtype=torch.uint8, device=dev)
                    dec(raw, fr)
                else:
                    fr = raw
                self.last_params, self.last_seed = params, seed
                if self.render is None:
                    yield augment_batch(fr[:bs], fr[bs:2 * bs], fr[2 * bs:], an, pr, mano_layer=self.mano_layer, seed=seed, augment=self.augment)
                    continue
                from ..utils.vis_utils import render_frames
                from .dataset import gt_batch
                gt = gt_batch(self.mano_layer, an)
                faces, colors, ws = self.render
                verts = torch.cat((gt[1], gt[3]), dim=1).contiguous()
                masks, dense = render_frames(verts, faces, gt[8], colors, S, workspace=ws)
                if self.round_trip is not None:
                    masks, dense = self.round_trip(masks), self.round_trip(dense)
                yield augment_batch(fr, masks, dense, gt, pr, seed=seed, augment=self.augment)
            if dec is not None:
                dec.check()                                                # a record that was not a 256x256 image would have left its frame stale
        finally:
            ring.close()
