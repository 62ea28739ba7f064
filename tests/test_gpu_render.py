"""GPU: the two-hand mesh rasteriser (csrc/render.hip through dir_amd.utils.vis_utils): bit-exact with the numpy restatement
(tests/helpers/raster_ref.py) on ground-truth meshes and on an adversarial scene, occlusion, determinism and graph replay, the
reference class's outputs, argument checks, TrainBatches with rendered targets and the render_split tool."""
import ctypes as C
import io
import json
import os
import pickle
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, 'helpers'))
import raster_ref as R  # noqa: E402
from fake_train_split import write_train_split  # noqa: E402

from dir_amd import _capi, synth  # noqa: E402
from dir_amd.apps import dataset as DS  # noqa: E402
from dir_amd.apps import trainset as T  # noqa: E402
from dir_amd.utils import vis_utils as V  # noqa: E402

pytestmark = pytest.mark.gpu

KEYS = ('pix_to_face', 'zbuf', 'bary', 'mask', 'color_u8', 'color_f32')


@pytest.fixture(scope='module')
def state():
    with open(os.path.join(HERE, 'golden', 'manifest_dir.json')) as fh:
        shapes = {k: tuple(v) for k, v in json.load(fh).items()}
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in synth.synth_state_dict(shapes, 1234).items()}


@pytest.fixture(scope='module')
def mano(state):
    return DS.gt_layers_from_checkpoint(state)


def dense_table(seed=7):
    return np.random.default_rng(seed).random((778, 3))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def gt_scene(mano, tmp, n=8, seed=3):
    """camera-frame meshes of the fake train split's annotations (gt_batch): verts [n,1556,3], K [n,3,3] on the GPU"""
    write_train_split(tmp, n, seed=seed)
    ds = DS.InterHandSplit(tmp, 'train')
    an = dev(np.stack([ds.anno(i) for i in range(n)]))
    gt = DS.gt_batch(mano, an)
    return torch.cat((gt[1], gt[3]), dim=1).contiguous(), gt[8].contiguous()


def reference(verts, faces, K, S, colors):
    v, f, k = verts.cpu().numpy(), faces.cpu().numpy(), K.cpu().numpy()
    with ThreadPoolExecutor(max_workers=8) as ex:                        # numpy releases the GIL on the big element-wise ops
        return list(ex.map(lambda b: R.render(v[b], f, k[b], S, colors), range(len(v))))


def assert_bit_exact(out, ref):
    for b, rb in enumerate(ref):
        for k in KEYS:
            got = out[k][b].cpu().numpy()
            want = rb[k].astype(got.dtype)
            assert got.shape == want.shape, k
            bad = (got.view(np.uint8) != want.view(np.uint8)).reshape(got.shape[0], got.shape[1], -1).any(-1)
            assert not bad.any(), (k, b, int(bad.sum()), np.argwhere(bad)[:4].tolist())


def run_all(verts, faces, K, S, colors):
    return V.rasterize(verts, faces, K, S, colors=colors, outputs=KEYS)


@pytest.mark.parametrize('S', [256, 224])
def test_ground_truth_meshes_bit_exact(tmp_path, mano, S):
    verts, K = gt_scene(mano, str(tmp_path))
    faces = torch.from_numpy(V.faces_from_layers(mano)).cuda()
    colors = V.load_dense_colors(dense_table())
    out = run_all(verts, faces, K, S, dev(colors))
    torch.cuda.synchronize()
    ref = reference(verts, faces, K, S, colors)
    assert_bit_exact(out, ref)
    p2f = out['pix_to_face'].cpu().numpy()
    assert (p2f >= 0).mean() > 0.02 and (p2f < 1538).any() and (p2f >= 1538).any()    # both hands in view


def adversarial_scene(S, seed=0):
    """zero-area faces, vertices behind the camera and at Z = 0, duplicated faces at equal depth, vertices on pixel centres, faces
    crossing tile borders and the image edge, one face larger than the image; K with fx = fy = 1, px = py = 0 (x_ndc = X / Z).
    Most faces are cells of a jittered 40 x 39 vertex grid over [-1.25, 1.25]^2, so that about half of the image stays open."""
    rng = np.random.default_rng(seed)
    B = 2
    K = np.tile(np.array([[-S / 2, 0, S / 2], [0, -S / 2, S / 2], [0, 0, 1]], np.float32), (B, 1, 1))
    i = np.arange(1556)
    xy = np.stack([-1.25 + (i % 40) * 2.5 / 39, -1.25 + (i // 40) * 2.5 / 38], -1)[None] + rng.uniform(-0.01, 0.01, (B, 1556, 2))
    z = 2.0 ** rng.integers(-1, 3, (B, 1556))                             # powers of two: X / Z is exact
    base = rng.integers(0, S - 9, (B, 100, 1, 2))
    pix = base + rng.integers(0, 9, (B, 100, 3, 2))                       # 100 small triangles with corners on pixel centres
    xy[:, :300] = (1 - (2 * pix + 1) / S).reshape(B, 300, 2)[..., ::-1]
    z[:, :300] = 1.0
    z[:, 300:340] = -z[:, 300:340]                                        # behind the camera
    z[:, 340:344] = 0.0                                                   # on the camera plane (non-finite projection)
    v = np.concatenate([xy * z[..., None], z[..., None]], -1).astype(np.float32)
    v[:, 1550:1553] = [[-40.0, -40.0, 8.0], [40.0, -40.0, 8.0], [0.0, 40.0, 8.0]]     # larger than the image, farthest
    v[:, 1553:1556] = [[0.2, 0.2, 1.0], [0.4, 0.2, 1.0], [0.6, 0.2, 1.0]]             # collinear: zero area
    cell = rng.integers(344, 1550 - 41, 3076)
    cell = cell - (cell % 40 == 39)
    up = rng.integers(0, 2, 3076).astype(bool)
    f = np.where(up[:, None], np.stack([cell, cell + 1, cell + 40], -1), np.stack([cell + 1, cell + 41, cell + 40], -1))
    f[:100] = np.arange(300).reshape(100, 3)                              # the pixel-centre triangles
    f[100:120] = rng.integers(0, 1556, (20, 3))                           # big random faces, special vertices included
    f[200:260] = f[1000:1060]                                             # earlier copies of later faces (equal depth: lower index wins)
    f[260:280, 1] = f[260:280, 0]                                         # repeated index: zero area
    f[280:300] = rng.integers(300, 344, (20, 3))                          # behind the camera / Z = 0
    f[300:340] = np.stack([rng.integers(344, 1500, 40), rng.integers(300, 340, 40), rng.integers(344, 1500, 40)], -1)   # one behind
    f[340:380] = np.stack([rng.integers(344, 1500, 40), rng.integers(300, 340, 40), rng.integers(300, 340, 40)], -1)   # two behind
    f[380:400] = np.stack([rng.integers(344, 1500, 20), rng.integers(340, 344, 20), rng.integers(344, 1500, 20)], -1)  # one at Z = 0
    f[1700:2400] = f[400:1100]                                            # fewer distinct cells: more of the big face stays visible
    f[3000] = [1550, 1551, 1552]
    f[3001] = [1551, 1550, 1552]                                          # the same triangle, other winding (pz rounds differently)
    f[3002] = [1553, 1554, 1555]
    return v, f.astype(np.int32), K


@pytest.mark.parametrize('S', [256, 100])
def test_adversarial_scene_bit_exact(S):
    v, f, K = adversarial_scene(S)
    colors = (np.random.default_rng(1).random((1556, 3)) * 255).astype(np.float32)
    out = run_all(dev(v), dev(f), dev(K), S, dev(colors))
    torch.cuda.synchronize()
    ref = reference(dev(v), dev(f), dev(K), S, colors)
    assert_bit_exact(out, ref)
    p2f = out['pix_to_face'].cpu().numpy()
    assert (p2f == 3000).any()                                            # the face larger than the image shows where nothing is nearer


def test_right_hand_in_front_occludes_the_left(tmp_path, mano):
    verts, K = gt_scene(mano, str(tmp_path), n=4, seed=5)
    faces = torch.from_numpy(V.faces_from_layers(mano)).cuda()
    vl = verts[:, :778]
    cl = vl.mean(1, keepdim=True)
    vr = vl - cl + cl * torch.tensor([1.0, 1.0, 0.9], device='cuda') + torch.tensor([0.01, 0.0, 0.0], device='cuda')   # nearer, shifted
    far = torch.tensor([1000.0, 0.0, 0.0], device='cuda')
    cov = {}
    for name, (a, b) in {'left': (vl, vr + far), 'right': (vl + far, vr), 'both': (vl, vr)}.items():
        cov[name] = V.rasterize(torch.cat((a, b), 1).contiguous(), faces, K, 256, outputs=('pix_to_face',))['pix_to_face']
    both = (cov['left'] >= 0) & (cov['right'] >= 0)
    assert int(both.sum()) > 500
    assert bool((cov['both'][both] >= 1538).all())


def test_two_runs_and_a_graph_replay_are_bit_identical(tmp_path, mano):
    verts, K = gt_scene(mano, str(tmp_path), n=4, seed=6)
    faces = torch.from_numpy(V.faces_from_layers(mano)).cuda()
    colors = dev(V.load_dense_colors(dense_table()))
    ws = torch.empty(int(_capi.lib().dir_render_workspace_bytes(4)), dtype=torch.uint8, device='cuda')
    a = V.rasterize(verts, faces, K, 256, colors=colors, outputs=KEYS, workspace=ws)
    b = V.rasterize(verts, faces, K, 256, colors=colors, outputs=KEYS, workspace=ws)
    torch.cuda.synchronize()
    for k in KEYS:
        assert torch.equal(a[k], b[k]), k
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        V.rasterize(verts, faces, K, 256, colors=colors, outputs=KEYS, workspace=ws)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g = V.rasterize(verts, faces, K, 256, colors=colors, outputs=KEYS, workspace=ws)
    for _ in range(2):
        for k in KEYS:
            g[k].zero_()
        graph.replay()
        torch.cuda.synchronize()
        for k in KEYS:
            assert torch.equal(a[k], g[k]), k


def test_reference_class_outputs(tmp_path, mano):
    verts, K = gt_scene(mano, str(tmp_path), n=2, seed=8)
    r = V.mano_two_hands_renderer(right_faces=mano['right'].get_faces(), dense_color=dense_table(), img_size=224, device='cuda')
    vl, vr = verts[:, :778], verts[:, 778:]
    mask = r.render_mask(cameras=K, v3d_left=vl, v3d_right=vr)
    img, alpha = r.render_densepose(cameras=K, v3d_left=vl, v3d_right=vr)
    depth = r.render_depth(cameras=K, v3d_left=vl, v3d_right=vr)
    torch.cuda.synchronize()
    assert mask.shape == (2, 224, 224, 3) and mask.dtype == torch.float32
    assert img.shape == (2, 224, 224, 3) and img.dtype == torch.float32 and alpha.shape == (2, 224, 224) and alpha.dtype == torch.float32
    assert depth.shape == (2, 224, 224, 1) and depth.dtype == torch.float32
    fg = alpha > 0
    bg_val = torch.tensor(1.0, dtype=torch.float32) / 255
    assert bool((mask[~fg] == bg_val.item()).all()) and bool((img[~fg] == bg_val.item()).all())
    assert bool((depth[..., 0][~fg] == -1).all()) and bool((depth[..., 0][fg] > 0).all())
    assert float(mask.max()) <= 1.0 + 1e-6 and float(mask[fg].sum(-1).min()) > 0.99           # one hand colour per pixel, 255 / 255
    assert float(img.max()) <= 1.0 + 1e-6 and float(img.min()) >= 0
    # the values: texel / 255 of the restatement
    ref = reference(verts, r.faces, K, 224, V.load_dense_colors(dense_table()))
    for b in range(2):
        np.testing.assert_array_equal(img[b].cpu().numpy(), ref[b]['color_f32'])
        np.testing.assert_array_equal(depth[b, ..., 0].cpu().numpy(), ref[b]['zbuf'])
    with pytest.raises(NotImplementedError):
        r.render_mask(scale=torch.ones(2), trans2d=torch.zeros(2, 2), v3d_left=vl, v3d_right=vr)
    with pytest.raises(NotImplementedError):
        r.render_rgb(cameras=K, v3d_left=vl, v3d_right=vr)


def test_bad_arguments(mano):
    rf = np.asarray(mano['right'].get_faces()).copy()
    rf[5, 1] = 778
    with pytest.raises(ValueError):
        V.two_hand_faces(rf)
    with pytest.raises(ValueError):
        V.mano_two_hands_renderer(right_faces=rf, dense_color=dense_table())
    B, S = 2, 64
    v, f, K = adversarial_scene(S, seed=4)
    vv, ff, KK = dev(v), dev(f), dev(K)
    with pytest.raises(ValueError):
        V.rasterize(vv.double(), ff, KK, S)
    with pytest.raises(ValueError):
        V.rasterize(vv, ff.long(), KK, S)
    with pytest.raises(ValueError):
        V.rasterize(vv[:, :1000].contiguous(), ff, KK, S)
    with pytest.raises(ValueError):
        V.rasterize(vv, ff, KK[:1].contiguous(), S)
    for bad in (15, 1025):
        with pytest.raises(ValueError):
            V.rasterize(vv, ff, KK, bad)
    L, P = _capi.lib(), _capi.ptr
    ws = torch.empty(int(L.dir_render_workspace_bytes(B)), dtype=torch.uint8, device='cuda')
    p2f = torch.empty(B, S, S, dtype=torch.int32, device='cuda')
    u8 = torch.empty(B, S, S, 3, dtype=torch.uint8, device='cuda')
    ok = [P(vv), P(ff), P(KK), None, B, S, P(ws), ws.numel(), P(p2f), None, None, None, None, None, None]
    assert L.dir_render_two_hands(*ok) == 0
    for pos, val in ((0, None), (1, None), (2, None), (6, None), (5, 15), (5, 1025), (4, -1), (4, 5000), (7, ws.numel() - 1), (8, None)):
        args = list(ok)
        args[pos] = val
        assert L.dir_render_two_hands(*args) < 0, (pos, val)
    args = list(ok)
    args[12] = P(u8)                                                      # a colour frame without the colour table
    assert L.dir_render_two_hands(*args) < 0
    # a face index outside the vertex table through the C ABI: the face is skipped, nothing is read out of bounds
    f2 = f.copy()
    f2[7] = [0, 1556, 2]
    f2[8] = [-1, 4, 5]
    f2[9] = [1 << 30, 4, 5]
    assert L.dir_render_two_hands(P(vv), P(dev(f2)), P(KK), None, B, S, P(ws), ws.numel(), P(p2f), None, None, None, None, None,
                                  None) == 0
    torch.cuda.synchronize()
    ref = [R.rasterize(v[b], f2, K[b], S)[0] for b in range(B)]
    np.testing.assert_array_equal(p2f.cpu().numpy(), np.stack(ref))
    assert L.dir_render_two_hands(P(vv), P(ff), P(KK), None, 0, S, None, 0, None, None, None, None, None, None, None) == 0   # empty batch


def test_train_batches_with_rendered_targets(tmp_path, state, mano):
    n, bs = 7, 3
    write_train_split(str(tmp_path), n, seed=9)
    for kind in ('mask', 'dense'):
        shutil.rmtree(str(tmp_path / 'train' / kind))                    # rendered, not read
    table = dense_table()
    tb = T.TrainBatches(str(tmp_path), mano, 'train', batch_size=bs, workers=2, seed=5, dense_color=table)
    ds = DS.InterHandSplit(str(tmp_path), 'train')
    faces = V.faces_from_layers(mano)
    colors = V.load_dense_colors(table)
    batches = 0
    for inputs, targets, meta in tb:
        torch.cuda.synchronize()
        P, seed = tb.last_params, tb.last_seed
        rows = []
        for b in range(bs):
            K = meta['camera'][b].cpu().numpy()
            idx = [i for i in range(n) if np.array_equal(ds.anno(i)[12:21].reshape(3, 3), K)]
            assert len(idx) == 1
            rows.append(idx[0])
        gt = DS.gt_batch(mano, dev(np.stack([ds.anno(i) for i in rows])))
        verts = torch.cat((gt[1], gt[3]), 1).cpu().numpy()
        Kn = gt[8].cpu().numpy()
        ref = [R.render(verts[b], faces, Kn[b], 256, colors) for b in range(bs)]
        m = dev(np.stack([r['mask'] for r in ref]))
        d = dev(np.stack([r['color_u8'] for r in ref]))
        z = torch.zeros_like(m)
        ri, rt, _ = T.augment_batch(z, m, d, gt, P, seed=seed)
        assert torch.equal(inputs['mask_rgb'], ri['mask_rgb'])
        assert torch.equal(targets['seg'], rt['seg']) and torch.equal(targets['dense'], rt['dense'])
        assert bool((targets['seg'] == 1).any()) and bool((targets['seg'] == 2).any())
        batches += 1
    assert batches == 2


def test_render_split_tool(tmp_path, state, mano):
    from PIL import Image
    n = 5
    root = str(tmp_path / 'data')
    write_train_split(root, n, seed=2)
    for kind in ('mask', 'dense'):
        shutil.rmtree(os.path.join(root, 'train', kind))
    ckpt, dense = str(tmp_path / 'ckpt.pt'), str(tmp_path / 'dense.pkl')
    torch.save(state, ckpt)
    table = dense_table(11)
    with open(dense, 'wb') as fh:
        pickle.dump(table, fh)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    r = subprocess.run([sys.executable, '-m', 'dir_amd.apps.render_split', '--save_path', root, '--model', ckpt, '--dense_color', dense,
                        '--bs', '2', '--workers', '2'], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    for kind in ('mask', 'dense'):
        assert sorted(os.listdir(os.path.join(root, 'train', kind))) == sorted('%d.jpg' % i for i in range(n))
    # the files: Pillow's own encode / decode of the rendered frames, in the renderer's channel order
    ds = DS.InterHandSplit(root, 'train')
    gt = DS.gt_batch(mano, dev(np.stack([ds.anno(i) for i in range(n)])))
    faces = torch.from_numpy(V.faces_from_layers(mano)).cuda()
    m, d = V.render_frames(torch.cat((gt[1], gt[3]), 1).contiguous(), faces, gt[8], dev(V.load_dense_colors(table)))
    for kind, fr in (('mask', m), ('dense', d)):
        for i in range(n):
            buf = io.BytesIO()
            Image.fromarray(np.ascontiguousarray(fr[i].cpu().numpy()[:, :, ::-1])).save(buf, format='JPEG', quality=95, subsampling=2)
            buf.seek(0)
            with Image.open(buf) as im:
                want = np.asarray(im.convert('RGB'))[:, :, ::-1]
            np.testing.assert_array_equal(DS.decode_bgr(ds.path(kind, i)), want, err_msg='%s %d' % (kind, i))
    # the file path of TrainBatches reads them
    for inputs, targets, meta in T.TrainBatches(root, mano, 'train', batch_size=2, workers=1, seed=0):
        torch.cuda.synchronize()
        assert inputs['img'].shape == (2, 3, 256, 256) and bool((targets['seg'] > 0).any())
        break


def test_render_split_needs_faces(tmp_path, state):
    write_train_split(str(tmp_path), 1, seed=1)
    from dir_amd.apps.render_split import render_split
    no_faces = {k: v for k, v in state.items() if not k.endswith('th_faces')}
    with pytest.raises(ValueError, match='th_faces'):
        render_split(str(tmp_path), no_faces, dense_table(), 'train', bs=2, workers=1)
    with pytest.raises(ValueError, match='th_faces'):
        T.TrainBatches(str(tmp_path), DS.gt_layers_from_checkpoint(no_faces), 'train', batch_size=1, workers=1, dense_color=dense_table())
