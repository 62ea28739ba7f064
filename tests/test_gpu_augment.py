"""GPU: the training input of dataset/interhand.py:__getitem__ (split 'train') -- csrc/augment.hip through dir_amd.apps.trainset.
Image pass bit-exact with the numpy restatement (tests/helpers/augment_ref.py), labels against the reference's own maths (G23), the noise
field, graph capture, argument checks, and TrainBatches from files end to end."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'helpers'))
import augment_ref as R  # noqa: E402
from fake_train_split import write_train_split  # noqa: E402

from dir_amd import _capi, synth  # noqa: E402
from dir_amd.apps import dataset as DS  # noqa: E402
from dir_amd.apps import trainset as T  # noqa: E402

pytestmark = pytest.mark.gpu

LABELS = ('joint_2d_left', 'mesh_2d_left', 'joint_2d_right', 'mesh_2d_right', 'joint_3d_left', 'mesh_3d_left', 'joint_3d_right', 'mesh_3d_right')


def frames(B, seed):
    rng = np.random.RandomState(seed)
    img = rng.randint(0, 256, (B, 256, 256, 3)).astype(np.uint8)
    yy, xx = np.mgrid[0:256, 0:256]
    mask = np.zeros((B, 256, 256, 3), np.uint8)
    for b in range(B):
        blob = (xx - 100 - 3 * b) ** 2 + (yy - 120) ** 2 < 60 ** 2
        mask[b, ..., 1] = np.where(blob, rng.randint(30, 256, (256, 256)), rng.randint(0, 60, (256, 256)))
        mask[b, ..., 2] = np.where(xx > 128, rng.randint(30, 256, (256, 256)), rng.randint(0, 70, (256, 256)))
    dense = rng.randint(0, 256, (B, 256, 256, 3)).astype(np.uint8)
    return img, mask, dense


def param_grid():
    """every blur size 3..9, flips, rot +-180 / 90, scale 0.9 / 1.1, tx / ty +-10, identity"""
    cases = [(0, 1.0, 0, 0, 0, 0), (180, 1.0, 0, 0, 1, 0), (-180, 0.9, 10, -10, 0, 3), (90, 1.1, -10, 10, 1, 4), (37.5, 0.95, 2.5, -7.25, 0, 5),
             (-123.4, 1.07, -3.3, 4.4, 1, 6), (12.0, 1.0, 0, 0, 0, 7), (0, 1.0, 0, 0, 1, 8), (-45, 0.9, 9.9, 9.9, 1, 9), (170, 1.1, -9.5, 0.5, 0, 0)]
    rng = np.random.default_rng(11)
    P = np.zeros(len(cases), T.AUG_DTYPE)
    for i, (rot, sc, tx, ty, flip, ks) in enumerate(cases):
        P['M'][i] = T.affine_mat(float(rot), sc, float(tx), float(ty))[:2].reshape(6)
        P['flip'][i] = flip
        if ks:
            P['blur'][i] = ks
            P['kernel'][i, :ks * ks] = T.motion_blur_kernel(ks, rng.uniform(-180, 180) * np.pi / 180).reshape(-1)
        P['a'][i] = rng.uniform(0.7, 1.3, 3)
        P['b'][i] = 12.75 * (2 * rng.random() - 1)
    P['a'][0], P['b'][0] = (1.0, 1.0, 1.0), 0.0
    return P


def label_inputs(g, cases):
    """G23's inputs (one set, shared by its cases) repeated for each case: the gt_batch tuple of a batch of len(cases)"""
    keys = ('joint_xyz_left', 'mesh_xyz_left', 'joint_xyz_right', 'mesh_xyz_right', 'joint_uv_left', 'mesh_uv_left', 'joint_uv_right',
            'mesh_uv_right', 'camera')
    return tuple(torch.from_numpy(np.stack([g['in.' + k] for _ in cases])).cuda() for k in keys)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def test_image_pass_bit_exact_with_the_restatement():
    P = param_grid()
    B = len(P)
    img, mask, dense = frames(B, 1)
    noise = (np.random.RandomState(2).standard_normal((B, 256, 256, 3)) * 2.55).astype(np.float32)
    noise[0, :8] = 300.0                          # clip at 255
    noise[0, 8:16] = -300.0                       # clip at 0
    g = np.load(os.path.join(HERE, 'golden', 'g23_train_aug.npz'))
    gt = label_inputs(g, range(B))
    inputs, targets, meta = T.augment_batch(dev(img), dev(mask), dev(dense), gt, P, noise=dev(noise))
    torch.cuda.synchronize()
    got = {'img_rgb': inputs['img_rgb'].cpu().numpy(), 'mask_rgb': inputs['mask_rgb'].cpu().numpy(), 'seg': targets['seg'].cpu().numpy(),
           'dense': targets['dense'].cpu().numpy(), 'img': inputs['img'].cpu().numpy()}
    for b in range(B):
        ref = R.augment_images(img[b], mask[b], dense[b], P[b], noise[b])
        for k in ('img_rgb', 'mask_rgb', 'seg', 'dense', 'img'):
            assert got[k][b].shape == ref[k].shape, k
            bad = int((got[k][b] != ref[k]).sum())
            assert bad == 0, (k, b, int(P['blur'][b]), bad)
    assert (got['seg'] == 1).any() and (got['seg'] == 2).any()
    # inputs['img'] is dir_image_normalize_forward of the noised frame, bit for bit
    u8 = inputs['img_rgb'].to(torch.uint8).contiguous()
    ref_img = torch.empty_like(inputs['img'])
    mean, std = (C.c_float * 3)(*T.MEAN), (C.c_float * 3)(*T.STD)
    _capi.check(_capi.lib().dir_image_normalize_forward(_capi.ptr(u8), _capi.ptr(ref_img), mean, std, B, 256, 256, _capi.stream_ptr()), 'norm')
    assert torch.equal(ref_img, inputs['img'])
    # the identity case with a = 1, b = 0: the noised input frame itself
    np.testing.assert_array_equal(got['img_rgb'][0][16:], np.clip(img[0].astype(np.float64) + noise[0], 0, 255).astype(np.uint8)[16:])


def test_labels_against_g23():
    g = dict(np.load(os.path.join(HERE, 'golden', 'g23_train_aug.npz')))
    B = int(g['cases'])
    P = np.zeros(B, T.AUG_DTYPE)
    for c in range(B):
        P['M'][c] = g['M.%d' % c][:2].reshape(6)
        P['flip'][c] = int(g['flip.%d' % c])
    gt = label_inputs(g, range(B))
    z = torch.zeros(B, 256, 256, 3, dtype=torch.uint8, device='cuda')
    _, targets, meta = T.augment_batch(z, z, z, gt, P)
    torch.cuda.synchronize()
    worst_uv, worst_xyz = 0.0, 0.0
    for c in range(B):
        for k in LABELS + ('center_left', 'center_right'):
            v = (meta if k.startswith('center') else targets)[k][c].cpu().numpy().astype(np.float64)
            if k.startswith('mesh'):
                v = v[g['vsub']]                                                # G23 keeps every 26th vertex row (and the last)
            ref = g['out.%d.%s' % (c, k)]
            if '_2d_' in k:
                e_uv = float(np.abs(v[:, :2] - ref[:, :2]).max()) * 128.0        # back to pixels
                e_z = float(np.abs(v[:, 2] - ref[:, 2]).max())
                assert e_uv <= 1e-4 and e_z <= 1e-7, (c, k, e_uv, e_z)
                worst_uv = max(worst_uv, e_uv)
            else:
                e = float(np.abs(v - ref).max())
                assert e <= 1e-7, (c, k, e)
                worst_xyz = max(worst_xyz, e)
    assert torch.equal(meta['camera'], gt[8])
    print('labels vs G23: max %.2e px on uv, %.2e m on xyz' % (worst_uv, worst_xyz))


def test_labels_pass_through_without_augmentation():
    g = dict(np.load(os.path.join(HERE, 'golden', 'g23_train_aug.npz')))
    gt = label_inputs(g, range(4))
    z = torch.zeros(4, 256, 256, 3, dtype=torch.uint8, device='cuda')
    P = T.sample_params(np.random.default_rng(0), 4, augment=False)
    _, targets, meta = T.augment_batch(z, z, z, gt, P, augment=False)
    assert torch.equal(targets['joint_3d_left'], gt[0]) and torch.equal(targets['mesh_3d_right'], gt[3])
    assert torch.equal(meta['center_right'], gt[2][:, 9:10])
    uv = (gt[4].double() / 256 * 2 - 1).float()
    assert torch.equal(targets['joint_2d_left'][..., :2], uv) and torch.equal(targets['joint_2d_left'][..., 2], gt[0][..., 2])


def test_noise_field_statistics_and_determinism():
    a = T.noise_field(1234, 8)
    b = T.noise_field(1234, 8)
    c = T.noise_field(1235, 8)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and not torch.equal(a, c)
    x = a.double()
    mean, std = float(x.mean()), float(x.std())
    assert abs(mean) < 0.01 and abs(std / 2.55 - 1) < 0.01, (mean, std)
    assert float((x.abs() > 3 * 2.55).double().mean()) < 0.004          # Gaussian tails (0.27 % beyond 3 sigma)
    # per channel and per image: no structure
    for ch in range(3):
        assert abs(float(x[..., ch].std()) / 2.55 - 1) < 0.01
    # the image pass with noise=None generates exactly this field
    P = param_grid()[:8]
    img, mask, dense = [dev(f) for f in frames(8, 3)]
    gt = label_inputs(dict(np.load(os.path.join(HERE, 'golden', 'g23_train_aug.npz'))), range(8))
    i1, t1, _ = T.augment_batch(img, mask, dense, gt, P, noise=None, seed=1234)
    i2, t2, _ = T.augment_batch(img, mask, dense, gt, P, noise=a)
    assert torch.equal(i1['img_rgb'], i2['img_rgb']) and torch.equal(i1['img'], i2['img'])


def test_augment_captures_in_a_graph_and_replays_bit_identically():
    P = param_grid()
    B = len(P)
    img, mask, dense = [dev(f) for f in frames(B, 4)]
    gt = label_inputs(dict(np.load(os.path.join(HERE, 'golden', 'g23_train_aug.npz'))), range(B))
    pd = T.params_to_device(P, 'cuda')
    scratch = torch.empty(B, 256, 256, 3, dtype=torch.uint8, device='cuda')
    eager = T.augment_batch(img, mask, dense, gt, pd, seed=77, scratch=scratch)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        T.augment_batch(img, mask, dense, gt, pd, seed=77, scratch=scratch)      # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = T.augment_batch(img, mask, dense, gt, pd, seed=77, scratch=scratch)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(eager, out):
            for k in a:
                assert torch.equal(a[k], b[k]), k


def test_bad_arguments_return_negative_codes():
    L = _capi.lib()
    x = torch.zeros(2, 256, 256, 3, dtype=torch.uint8, device='cuda')
    f = torch.zeros(2, 3, 256, 256, device='cuda')
    p = T.params_to_device(T.sample_params(np.random.default_rng(0), 2), 'cuda')
    mean, std = (C.c_float * 3)(*T.MEAN), (C.c_float * 3)(*T.STD)
    P = _capi.ptr
    ok = (P(p), P(x), P(x), P(x), None, C.c_ulonglong(1), mean, std, P(x), P(f), None, None, P(f), P(f), 2, None)
    for pos in (0, 1, 2, 3, 8, 9, 12, 13):
        args = list(ok)
        args[pos] = None
        assert L.dir_train_augment_images(*args) < 0, pos
    args = list(ok)
    args[14] = -1
    assert L.dir_train_augment_images(*args) < 0
    args[14] = 1 << 20
    assert L.dir_train_augment_images(*args) < 0
    args = list(ok)
    args[7] = (C.c_float * 3)(1, 0, 1)
    assert L.dir_train_augment_images(*args) < 0
    assert L.dir_train_noise_field(C.c_ulonglong(0), None, 2, None) < 0
    assert L.dir_train_noise_field(C.c_ulonglong(0), P(f), -3, None) < 0
    ins = (C.c_void_p * 8)(*([P(f)] * 7 + [None]))
    outs = (C.c_void_p * 10)(*([P(f)] * 10))
    assert L.dir_train_augment_labels(P(p), C.byref(ins), P(f), C.byref(outs), 2, None) < 0
    ins = (C.c_void_p * 8)(*([P(f)] * 8))
    assert L.dir_train_augment_labels(P(p), C.byref(ins), None, C.byref(outs), 2, None) < 0
    assert L.dir_train_augment_labels(P(p), None, P(f), C.byref(outs), 2, None) < 0
    assert L.dir_train_augment_labels(P(p), C.byref(ins), P(f), C.byref(outs), 0, None) == 0        # empty batch: nothing to do
    torch.cuda.synchronize()


@pytest.fixture(scope='module')
def state():
    with open(os.path.join(HERE, 'golden', 'manifest_dir.json')) as fh:
        shapes = {k: tuple(v) for k, v in json.load(fh).items()}
    return synth.synth_state_dict(shapes, 1234)


@pytest.mark.parametrize('records', [True, False])
def test_train_batches_equal_the_per_sample_restatement(tmp_path, state, records):
    n, bs = 7, 3
    write_train_split(str(tmp_path), n, seed=9)
    mano = DS.gt_layers_from_checkpoint({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in state.items()})
    tb = T.TrainBatches(str(tmp_path), mano, 'train', batch_size=bs, workers=2, seed=5, records=records)
    assert len(tb) == 2                                                  # drop_last
    ds = DS.InterHandSplit(str(tmp_path), 'train')
    seen = []
    for _ in range(2):                                                   # two epochs: a new permutation each
        rows = []
        for inputs, targets, meta in tb:
            torch.cuda.synchronize()
            P, seed = tb.last_params, tb.last_seed
            noise = T.noise_field(seed, bs).cpu().numpy()
            # each row's file index, from its camera (fake_split gives every index its own focal length)
            for b in range(bs):
                K = meta['camera'][b].cpu().numpy()
                idx = [i for i in range(n) if np.array_equal(ds.anno(i)[12:21].reshape(3, 3), K)]
                assert len(idx) == 1
                i = idx[0]
                rows.append(i)
                ref = R.augment_images(DS.decode_bgr(ds.path('img', i)), DS.decode_bgr(ds.path('mask', i)), DS.decode_bgr(ds.path('dense', i)),
                                       P[b], noise[b])
                for k in ('img', 'img_rgb', 'mask_rgb'):
                    np.testing.assert_array_equal(inputs[k][b].cpu().numpy(), ref[k], err_msg=k)
                for k in ('seg', 'dense'):
                    np.testing.assert_array_equal(targets[k][b].cpu().numpy(), ref[k], err_msg=k)
                an = torch.from_numpy(ds.anno(i)[None]).cuda()
                gt = [t[0].double().cpu().numpy() for t in DS.gt_batch(mano, an)]
                lab = R.augment_labels(*gt, P[b])
                for k in LABELS:
                    e = np.abs(targets[k][b].cpu().numpy() - lab[k]).max()
                    assert e < 1e-5, (k, e)
                for k in ('center_left', 'center_right'):
                    assert np.abs(meta[k][b].cpu().numpy() - lab[k]).max() < 1e-5
        assert len(rows) == 2 * bs and len(set(rows)) == len(rows)
        seen.append(rows)
    assert seen[0] != seen[1]


def test_two_train_steps_on_train_batches(tmp_path, state):
    from dir_amd.optim import FlatAdamW
    from dir_amd.train import step as TSTEP
    n, bs = 4, 2
    write_train_split(str(tmp_path), n, seed=4)
    sd = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in state.items()}
    mano = DS.gt_layers_from_checkpoint(sd)
    is_buf = lambda k: any(t in k for t in ('running_', 'num_batches', 'mano_layer', 'img_gird', 'seg_loss.weight'))  # noqa: E731
    params = {k: torch.nn.Parameter(v.cuda()) for k, v in sd.items() if not is_buf(k)}
    buffers = {k: v.cuda() for k, v in sd.items() if is_buf(k) and 'num_batches' not in k}
    opt = FlatAdamW(list(params.values()), lr=1e-5)
    opt.set_inactive(TSTEP.inactive_parameters(params))
    before = {k: p.detach().clone() for k, p in params.items()}
    faces = tuple(buffers['init_regressor.mano_layer_%s.th_faces' % s].long() for s in ('left', 'right'))
    losses = []
    for inputs, targets, meta in T.TrainBatches(str(tmp_path), mano, 'train', batch_size=bs, workers=2, seed=1):
        loss = TSTEP.train_step(params, buffers, inputs['img'], targets, meta, faces, opt)
        losses.append(sum(float(v) for v in loss.values()))
    assert len(losses) == 2 and all(np.isfinite(losses)), losses
    assert sum(int(not torch.equal(p.detach(), before[k])) for k, p in params.items()) > 0
