"""GPU: shaded and orthographic rendering (dir_render_shaded / dir_render_vertex_normals / dir_render_joints through
dir_amd.utils.vis_utils): bit-exact with the numpy restatement (tests/helpers/shade_ref.py) on ground-truth meshes and on an adversarial
scene, consistency with the existing rasteriser, the overlay rule, repeatability and graph replay, the subclass's API, argument checks,
overlay_predictions and the visualize command.  Parity is to the restatement, unpinned against pytorch3d (not installed; and it composes
its camera transforms as 4x4 matrix products, so with it equality would be to rounding only)."""
import json
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, 'helpers'))
import raster_ref as R  # noqa: E402
import shade_ref as SH  # noqa: E402
from fake_split import write_split  # noqa: E402
from fake_train_split import write_train_split  # noqa: E402

from dir_amd import _capi, synth  # noqa: E402
from dir_amd.apps import dataset as DS  # noqa: E402
from dir_amd.utils import vis_utils as V  # noqa: E402

pytestmark = pytest.mark.gpu

KEYS = ('pix_to_face', 'zbuf', 'bary', 'shaded_f32', 'overlay_u8')
LIGHT = SH.POINT_LIGHT


@pytest.fixture(scope='module')
def state():
    with open(os.path.join(HERE, 'golden', 'manifest_dir.json')) as fh:
        shapes = {k: tuple(v) for k, v in json.load(fh).items()}
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in synth.synth_state_dict(shapes, 1234).items()}


@pytest.fixture(scope='module')
def mano(state):
    return DS.gt_layers_from_checkpoint(state)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def gt_scene(mano, tmp, n, seed):
    """camera-frame meshes of the fake train split's annotations, as test_gpu_render.py builds them"""
    write_train_split(tmp, n, seed=seed)
    ds = DS.InterHandSplit(tmp, 'train')
    gt = DS.gt_batch(mano, dev(np.stack([ds.anno(i) for i in range(n)])))
    return torch.cat((gt[1], gt[3]), dim=1).contiguous(), gt[8].contiguous()


def framing_cameras(verts, fill=0.8):
    """orthographic cameras that keep both hands in view: the two-hand box of every image centred, its longer side `fill` of the picture"""
    v = verts.cpu().numpy().astype(np.float64)[..., :2]
    lo, hi = v.min(1), v.max(1)
    scale = 2 * fill / (hi - lo).max(-1) / 2                              # 2 * scale * extent = fill of the NDC range, which is 2 wide
    trans = -2 * scale[:, None] * (lo + hi) / 2
    return scale.astype(np.float32), trans.astype(np.float32)


def reference(verts, faces, S, colors, K=None, scale=None, trans2d=None, lights=LIGHT, background=None):
    v, f = verts.cpu().numpy(), faces.cpu().numpy()

    def one(b):
        kw = dict(K=K[b]) if K is not None else dict(scale=scale[b], trans2d=trans2d[b])
        return SH.render(v[b], f, S, colors, lights=lights, background=None if background is None else background[b], **kw)
    with ThreadPoolExecutor(max_workers=8) as ex:
        return list(ex.map(one, range(len(v))))


def assert_bit_exact(out, ref, keys=KEYS):
    for b, rb in enumerate(ref):
        for k in keys:
            got = out[k][b].cpu().numpy()
            want = rb[k].astype(got.dtype)
            assert got.shape == want.shape, k
            bad = (got.view(np.uint8) != want.view(np.uint8)).reshape(got.shape[0], got.shape[1], -1).any(-1)
            assert not bad.any(), (k, b, int(bad.sum()), np.argwhere(bad)[:4].tolist())


def both_hands_in_view(p2f):
    p = p2f.cpu().numpy()
    assert ((p >= 0) & (p < 1538)).mean() > 0.02 and (p >= 1538).mean() > 0.02


@pytest.mark.parametrize('S', [256, 224])
def test_ground_truth_meshes_bit_exact(tmp_path, mano, S):
    n = 3
    verts, K = gt_scene(mano, str(tmp_path), n, seed=3)
    faces = torch.from_numpy(V.faces_from_layers(mano)).cuda()
    colors = V.default_colors()
    frames = np.random.default_rng(S).integers(0, 256, (n, S, S, 3)).astype(np.uint8)
    normals = V.vertex_normals(verts, faces)
    torch.cuda.synchronize()
    v, f = verts.cpu().numpy(), faces.cpu().numpy()
    want_n = np.stack([SH.vertex_normals(v[b], f) for b in range(n)])
    assert np.array_equal(normals.cpu().numpy().view(np.uint32), want_n.view(np.uint32))
    length = np.linalg.norm(want_n, axis=-1)                             # unit normals; a vertex that the face table never names keeps a zero one
    used = np.zeros(1556, bool)
    used[np.unique(f)] = True
    assert np.abs(length[:, used] - 1).max() < 1e-5 and not want_n[:, ~used].any() and used.mean() > 0.5
    # the perspective camera
    out = V.rasterize_shaded(verts, faces, S, colors=dev(colors), K=K, background=dev(frames), outputs=KEYS)
    torch.cuda.synchronize()
    assert_bit_exact(out, reference(verts, faces, S, colors, K=K.cpu().numpy(), background=frames))
    # orthographic cameras that keep both hands in view
    scale, trans = framing_cameras(verts)
    out = V.rasterize_shaded(verts, faces, S, colors=dev(colors), scale=dev(scale), trans2d=dev(trans), background=dev(frames), outputs=KEYS)
    torch.cuda.synchronize()
    both_hands_in_view(out['pix_to_face'])
    assert_bit_exact(out, reference(verts, faces, S, colors, scale=scale, trans2d=trans, background=frames))
    # the light does something: the shaded picture is not the ambient one, and no channel leaves the colour scale by much
    amb = V.rasterize_shaded(verts, faces, S, colors=dev(colors), scale=dev(scale), trans2d=dev(trans), lights=V.AMBIENT_LIGHT)['shaded_f32']
    fg = out['pix_to_face'] >= 0
    assert float((out['shaded_f32'] - amb)[fg].abs().max()) > 0.05 and float(out['shaded_f32'].max()) < 1.01


def adversarial_scene(S, seed=0):
    """for the camera scale 0.5, trans2d 0 (x_ndc = -x): a jittered 40 x 39 vertex grid over [-1.25, 1.25]^2, so that the mesh is half out
    of the frame; 100 small triangles with corners on pixel centres; duplicated faces at equal depth; zero-area faces (repeated index,
    collinear) whose own vertices keep a zero normal; one face larger than the image; faces behind the camera plane (z + 10 < 0);
    a face index outside the table"""
    rng = np.random.default_rng(seed)
    B = 2
    i = np.arange(1556)
    xy = np.stack([-1.25 + (i % 40) * 2.5 / 39, -1.25 + (i // 40) * 2.5 / 38], -1)[None] + rng.uniform(-0.01, 0.01, (B, 1556, 2))
    z = rng.uniform(-0.5, 0.5, (B, 1556))
    pix = rng.integers(0, S - 9, (B, 100, 1, 2)) + rng.integers(0, 9, (B, 100, 3, 2))
    xy[:, :300] = -(1 - (2 * pix + 1) / S).reshape(B, 300, 2)
    z[:, :300] = 0.25
    z[:, 300:340] = -12.0                                                 # behind the camera plane: depth z + 10 < 0
    v = np.concatenate([xy, z[..., None]], -1).astype(np.float32)
    v[:, 1547:1550] = [[-40.0, -40.0, 3.0], [40.0, -40.0, 3.0], [0.0, 40.0, 3.0]]      # larger than the image, farthest
    v[:, 1550:1553] = [[0.2, 0.2, 1.0], [0.4, 0.2, 1.0], [0.6, 0.2, 1.0]]              # collinear: zero area, zero normals
    v[:, 1553:1556] = [[0.3, 0.3, 0.0], [0.3, 0.3, 0.0], [0.5, 0.1, 0.0]]              # used by a repeated-index face only
    cell = rng.integers(344, 1547 - 41, 3076)
    cell = cell - (cell % 40 == 39)
    up = rng.integers(0, 2, 3076).astype(bool)
    f = np.where(up[:, None], np.stack([cell, cell + 1, cell + 40], -1), np.stack([cell + 1, cell + 41, cell + 40], -1))
    f[:100] = np.arange(300).reshape(100, 3)
    f[100:120] = rng.integers(0, 1547, (20, 3))                           # big random faces
    f[200:260] = f[1000:1060]                                             # earlier copies of later faces: the lower index wins
    f[260:280, 1] = f[260:280, 0]                                         # repeated index: zero area
    f[280:300] = rng.integers(300, 340, (20, 3))                          # wholly behind the camera plane
    f[300:340] = np.stack([rng.integers(344, 1500, 40), rng.integers(300, 340, 40), rng.integers(344, 1500, 40)], -1)   # one vertex behind
    f[1700:2400] = f[400:1100]
    f[3000] = [1547, 1548, 1549]
    f[3001] = [1548, 1547, 1549]                                          # the same triangle, other winding
    f[3002] = [1550, 1551, 1552]
    f[3003] = [1553, 1553, 1555]
    f[3004] = [0, 1556, 2]                                                # outside the table: skipped
    return v, f.astype(np.int32)


@pytest.mark.parametrize('S', [256, 100])
def test_adversarial_scene_bit_exact(S):
    v, f = adversarial_scene(S)
    B = len(v)
    colors = (np.random.default_rng(1).random((1556, 3)) * 255).astype(np.float32)
    frames = np.random.default_rng(2).integers(0, 256, (B, S, S, 3)).astype(np.uint8)
    scale, trans = np.full(B, 0.5, np.float32), np.zeros((B, 2), np.float32)
    normals = V.vertex_normals(dev(v), dev(f)).cpu().numpy()
    want_n = np.stack([SH.vertex_normals(v[b], f) for b in range(B)])
    assert np.array_equal(normals.view(np.uint32), want_n.view(np.uint32))
    assert not normals[:, 1550:1556].any()                               # a zero normal stays zero
    out = V.rasterize_shaded(dev(v), dev(f), S, colors=dev(colors), scale=dev(scale), trans2d=dev(trans), background=dev(frames), outputs=KEYS)
    torch.cuda.synchronize()
    assert_bit_exact(out, reference(dev(v), dev(f), S, colors, scale=scale, trans2d=trans, background=frames))
    p2f = out['pix_to_face'].cpu().numpy()
    assert ((p2f == 3000) | (p2f == 3001)).any() and 0.2 < (p2f >= 0).mean()
    assert not np.isin(p2f, np.arange(280, 300)).any()                    # pz < 0 is skipped
    # the perspective camera on the same table (x_ndc = X / Z), pushed in front of the camera
    vp = v.copy()
    vp[..., 2] += 1.5
    vp[:, 300:340, 2] = -1.0
    K = np.tile(np.array([[-S / 2, 0, S / 2], [0, -S / 2, S / 2], [0, 0, 1]], np.float32), (B, 1, 1))
    out = V.rasterize_shaded(dev(vp), dev(f), S, colors=dev(colors), K=dev(K), background=dev(frames), outputs=KEYS)
    torch.cuda.synchronize()
    assert_bit_exact(out, reference(dev(vp), dev(f), S, colors, K=K, background=frames))


def test_ambient_and_perspective_agree_with_the_existing_entry_point(tmp_path, mano):
    verts, K = gt_scene(mano, str(tmp_path), 4, seed=5)
    faces = torch.from_numpy(V.faces_from_layers(mano)).cuda()
    colors = dev(V.load_dense_colors(np.random.default_rng(7).random((778, 3))))
    old = V.rasterize(verts, faces, K, 256, colors=colors, outputs=('pix_to_face', 'zbuf', 'bary', 'color_f32', 'color_u8'))
    new = V.rasterize_shaded(verts, faces, 256, colors=colors, K=K, lights=V.AMBIENT_LIGHT, outputs=KEYS)
    lit = V.rasterize_shaded(verts, faces, 256, colors=colors, K=K, outputs=KEYS)
    torch.cuda.synchronize()
    assert int((old['pix_to_face'] >= 0).sum()) > 2000
    for k in ('pix_to_face', 'zbuf', 'bary'):
        assert torch.equal(old[k], new[k]) and torch.equal(old[k], lit[k]), k
    assert torch.equal(old['color_f32'].view(torch.int32), new['shaded_f32'].view(torch.int32))
    assert torch.equal(old['color_u8'], new['overlay_u8'])                # no frame given: the background is the byte 1


def test_overlay_bytes(tmp_path, mano):
    S = 256
    verts, _ = gt_scene(mano, str(tmp_path), 3, seed=6)
    faces = torch.from_numpy(V.faces_from_layers(mano)).cuda()
    scale, trans = framing_cameras(verts)
    frames = dev(np.random.default_rng(3).integers(0, 256, (3, S, S, 3)).astype(np.uint8))
    o = V.rasterize_shaded(verts, faces, S, colors=dev(V.default_colors()), scale=dev(scale), trans2d=dev(trans), background=frames,
                           outputs=('pix_to_face', 'shaded_f32', 'overlay_u8'))
    torch.cuda.synchronize()
    fg = (o['pix_to_face'] >= 0).cpu().numpy()
    ov, sh = o['overlay_u8'].cpu().numpy(), o['shaded_f32'].cpu().numpy()
    assert 0.04 < fg.mean() < 0.9
    assert np.array_equal(ov[~fg], frames.cpu().numpy()[~fg])             # every background pixel carries the frame's bytes
    want = np.rint(np.clip(sh * np.float32(255), 0, 255)).astype(np.uint8)  # round_half_even(clamp(fl32(colour / 255) * 255, 0, 255))
    assert np.array_equal(ov[fg], want[fg])


def test_two_runs_and_a_graph_replay_are_bit_identical(tmp_path, mano):
    verts, _ = gt_scene(mano, str(tmp_path), 4, seed=6)
    faces = torch.from_numpy(V.faces_from_layers(mano)).cuda()
    colors = dev(V.default_colors())
    scale, trans = (dev(a) for a in framing_cameras(verts))
    frames = dev(np.random.default_rng(4).integers(0, 256, (4, 256, 256, 3)).astype(np.uint8))
    ws = torch.empty(int(_capi.lib().dir_render_shaded_workspace_bytes(4)), dtype=torch.uint8, device='cuda')

    def run():
        return V.rasterize_shaded(verts, faces, 256, colors=colors, scale=scale, trans2d=trans, background=frames, outputs=KEYS, workspace=ws)
    a, b = run(), run()
    n1, n2 = V.vertex_normals(verts, faces), V.vertex_normals(verts, faces)
    torch.cuda.synchronize()
    assert torch.equal(n1, n2)
    for k in KEYS:
        assert torch.equal(a[k], b[k]), k
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g = run()
    for _ in range(2):
        for k in KEYS:
            g[k].zero_()
        graph.replay()
        torch.cuda.synchronize()
        for k in KEYS:
            assert torch.equal(a[k], g[k]), k


def test_class_api(tmp_path, mano):
    S, n = 224, 2
    verts, K = gt_scene(mano, str(tmp_path), n, seed=8)
    table = np.random.default_rng(7).random((778, 3))
    kw = dict(right_faces=mano['right'].get_faces(), dense_color=table, img_size=S, device='cuda')
    r, base = V.mano_two_hands_shaded_renderer(**kw), V.mano_two_hands_renderer(**kw)
    vl, vr = verts[:, :778], verts[:, 778:]
    scale, trans = (dev(a) for a in framing_cameras(verts))
    bg = (torch.tensor(1.0) / 255).item()
    # render_rgb under both cameras: shapes, scales, and the values of the restatement
    for cam, ref_kw in ((dict(cameras=K), dict(K=K.cpu().numpy())), (dict(scale=scale, trans2d=trans), dict(scale=scale.cpu().numpy(), trans2d=trans.cpu().numpy()))):
        img, alpha = r.render_rgb(v3d_left=vl, v3d_right=vr, **cam)
        torch.cuda.synchronize()
        assert img.shape == (n, S, S, 3) and img.dtype == torch.float32 and alpha.shape == (n, S, S) and alpha.dtype == torch.float32
        fg = alpha > 0
        assert bool((img[~fg] == bg).all()) and bool(((alpha == 0) | (alpha == 1)).all()) and 0.02 < float(alpha.mean())
        assert float(img.min()) >= 0 and float(img.max()) < 1.01
        ref = reference(verts, r.faces, S, V.default_colors(), **ref_kw)
        for b in range(n):
            np.testing.assert_array_equal(img[b].cpu().numpy(), ref[b]['shaded_f32'])
            np.testing.assert_array_equal(alpha[b].cpu().numpy() > 0, ref[b]['pix_to_face'] >= 0)
    # amblights / v_color / lights
    img_a, _ = r.render_rgb(cameras=K, v3d_left=vl, v3d_right=vr, v_color=r.dense_coor, amblights=True)
    dense, _ = base.render_densepose(cameras=K, v3d_left=vl, v3d_right=vr)
    assert torch.equal(img_a, dense)
    img_l, _ = r.render_rgb(cameras=K, v3d_left=vl, v3d_right=vr, v_color=(10, 20, 30), lights=V.Lights(0.2, 0.5, 0.3, (0.1, 0.0, -0.5)))
    assert img_l.shape == (n, S, S, 3) and not torch.equal(img_l, img_a)
    # the orthographic camera in the inherited methods: texel / 255, background 1 / 255, depth z + 10 with -1 background
    mask = r.render_mask(scale=scale, trans2d=trans, v3d_left=vl, v3d_right=vr)
    dimg, dalpha = r.render_densepose(scale=scale, trans2d=trans, v3d_left=vl, v3d_right=vr)
    depth = r.render_depth(scale=scale, trans2d=trans, v3d_left=vl, v3d_right=vr)
    torch.cuda.synchronize()
    fg = dalpha > 0
    assert mask.shape == (n, S, S, 3) and dimg.shape == (n, S, S, 3) and dalpha.shape == (n, S, S) and depth.shape == (n, S, S, 1)
    assert bool((mask[~fg] == bg).all()) and bool((dimg[~fg] == bg).all()) and float(mask[fg].sum(-1).min()) > 0.9
    assert bool((depth[..., 0][~fg] == -1).all()) and bool((depth[..., 0][fg] > 9).all())
    o = V.rasterize_shaded(verts, r.faces, S, colors=r.dense_coor, scale=scale, trans2d=trans, lights=V.AMBIENT_LIGHT, outputs=('shaded_f32', 'zbuf'))
    assert torch.equal(dimg, o['shaded_f32']) and torch.equal(depth[..., 0], o['zbuf'])
    # and the perspective camera in them is the base class's path
    assert torch.equal(r.render_mask(cameras=K, v3d_left=vl, v3d_right=vr), base.render_mask(cameras=K, v3d_left=vl, v3d_right=vr))
    assert torch.equal(r.render_depth(cameras=K, v3d_left=vl, v3d_right=vr), base.render_depth(cameras=K, v3d_left=vl, v3d_right=vr))
    # render_rgb_orth = render_rgb on the remapped vertices
    sr, tr = scale * 1.25, trans + 0.1
    keep = vr.clone()
    img_o, alpha_o = r.render_rgb_orth(scale_left=scale, trans2d_left=trans, scale_right=sr, trans2d_right=tr, v3d_left=vl, v3d_right=vr)
    assert torch.equal(vr, keep)                                          # the caller's vertices are left alone
    moved = np.stack([SH.remap_right_hand(*(t[b].cpu().numpy() for t in (scale, trans, sr, tr)), vr[b].cpu().numpy()) for b in range(n)])
    assert float((V.remap_right_hand(scale, trans, sr, tr, vr).cpu() - torch.from_numpy(moved)).abs().max()) < 1e-6
    img_r, alpha_r = r.render_rgb(scale=scale, trans2d=trans, v3d_left=vl, v3d_right=V.remap_right_hand(scale, trans, sr, tr, vr))
    assert torch.equal(img_o, img_r) and torch.equal(alpha_o, alpha_r) and not torch.equal(img_o, r.render_rgb(scale=scale, trans2d=trans, v3d_left=vl, v3d_right=vr)[0])
    # refusals
    with pytest.raises(ValueError):
        r.render_rgb(cameras=K, scale=scale, trans2d=trans, v3d_left=vl, v3d_right=vr)
    with pytest.raises(ValueError):
        r.render_rgb(v3d_left=vl, v3d_right=vr)
    with pytest.raises(NotImplementedError):
        r.render_rgb(cameras=K, v3d_left=vl, v3d_right=vr, texture=torch.zeros(1, 8, 8, 3))
    # the base class behaves exactly as before
    with pytest.raises(NotImplementedError):
        base.render_mask(scale=scale, trans2d=trans, v3d_left=vl, v3d_right=vr)
    with pytest.raises(NotImplementedError):
        base.render_rgb(cameras=K, v3d_left=vl, v3d_right=vr)
    with pytest.raises(NotImplementedError):
        base.render_rgb_orth(scale_left=scale, trans2d_left=trans, scale_right=sr, trans2d_right=tr, v3d_left=vl, v3d_right=vr)


def test_bad_arguments():
    S, B = 64, 2
    v, f = adversarial_scene(S, seed=4)
    vv, ff = dev(v), dev(f)
    colors = dev(V.default_colors())
    scale, trans, K = torch.full((B,), 0.5, device='cuda'), torch.zeros(B, 2, device='cuda'), torch.eye(3, device='cuda').repeat(B, 1, 1)
    with pytest.raises(ValueError):
        V.rasterize_shaded(vv, ff, S, colors=colors, K=K, scale=scale, trans2d=trans)
    with pytest.raises(ValueError):
        V.rasterize_shaded(vv, ff, S, colors=colors)
    with pytest.raises(ValueError):
        V.rasterize_shaded(vv, ff, S, scale=scale, trans2d=trans)        # a colour output without colours
    with pytest.raises(ValueError):
        V.rasterize_shaded(vv, ff, S, colors=colors, scale=scale[:1].contiguous(), trans2d=trans)
    for bad in (15, 1025):
        with pytest.raises(ValueError):
            V.rasterize_shaded(vv, ff, bad, colors=colors, scale=scale, trans2d=trans)
    with pytest.raises(ValueError):
        V.rasterize_shaded(vv, ff, S, colors=colors, scale=scale, trans2d=trans, background=torch.zeros(B, S, S, 3, dtype=torch.uint8, device='cuda'))
    with pytest.raises(ValueError):
        V.vertex_normals(vv.double(), ff)
    # through the C ABI, with real pointers: a good call, then each broken one returns a negative code and launches nothing
    L, P = _capi.lib(), _capi.ptr
    adj = V.face_adjacency(ff)
    ws = torch.empty(int(L.dir_render_shaded_workspace_bytes(B)), dtype=torch.uint8, device='cuda')
    img = torch.empty(B, S, S, 3, device='cuda')
    lights = V.POINT_LIGHT.struct()
    ok = [P(vv), P(ff), P(adj), None, P(scale), P(trans), P(colors), lights, None, B, S, P(ws), ws.numel(), None, None, None, P(img), None, None]
    assert L.dir_render_shaded(*ok) == 0
    for pos, val in ((3, P(K)), (4, None), (0, None), (1, None), (2, None), (6, None), (7, None), (11, None), (10, 15), (10, 1025), (9, -1), (9, 5000),
                     (12, ws.numel() - 1), (16, None)):
        args = list(ok)
        args[pos] = val
        assert L.dir_render_shaded(*args) < 0 and L.dir_last_error(), (pos, val)
    args = list(ok)
    args[4] = args[5] = None                                              # no camera at all
    assert L.dir_render_shaded(*args) < 0
    args = list(ok)
    args[9], args[0], args[11], args[12] = 0, None, None, 0               # an empty batch is a no-op
    assert L.dir_render_shaded(*args) == 0
    torch.cuda.synchronize()
    assert V.rasterize_shaded(vv[:0].contiguous(), ff, S, colors=colors, scale=scale[:0].contiguous(), trans2d=trans[:0].contiguous())['shaded_f32'].shape == (0, S, S, 3)


def test_overlay_predictions(tmp_path, mano):
    """a constructed stage dict: ground-truth meshes (moved to the origin, as the network's root-relative meshes are) plus chosen pd_proj.
    For every covered pixel, DIR's own projection uv = s * xy + t of the ORIGINAL vertices, interpolated with the barycentrics, gives the
    pixel centre -- with the left hand's (s, t) on left-hand faces and the right hand's on right-hand faces, which checks the factor
    2 between DIR's scale and the camera's and the move of the right hand into the left camera.

    Tolerance per pixel: b_i = e_i / (area + 1e-8) shrinks the reconstruction by area / (area + 1e-8), at most 1e-8 / area for |centre| < 1,
    and each e_i is a difference of two products below 0.1^2 in size whose float32 rounding (3 * 2^-24 * 0.01 < 1e-8) is divided by the
    same area; the hands' faces are small (area 1e-5 .. 1e-3 in edge-function units), so the bound is 1e-5 + 2e-8 / area, per face."""
    S, n = 256, 4
    verts, _ = gt_scene(mano, str(tmp_path), n, seed=9)
    vl, vr = verts[:, :778].clone(), verts[:, 778:].clone()
    vl -= vl.mean(1, keepdim=True)
    vr -= vr.mean(1, keepdim=True)
    ext = float(torch.cat((vl, vr), 1)[..., :2].abs().max())
    s_l = torch.tensor([0.6, 0.7, 0.55, 0.75], device='cuda') / ext
    s_r = torch.tensor([0.7, 0.5, 0.6, 0.55], device='cuda') / ext
    t_l = torch.tensor([[-0.3, -0.2], [-0.25, 0.1], [0.0, -0.3], [-0.3, 0.0]], device='cuda')
    t_r = torch.tensor([[0.3, 0.2], [0.3, -0.1], [0.1, 0.35], [0.3, 0.1]], device='cuda')
    outs = {'pd_mesh_xyz_left': vl, 'pd_mesh_xyz_right': vr, 'pd_proj_left': torch.cat((s_l[:, None], t_l), 1),
            'pd_proj_right': torch.cat((s_r[:, None], t_r), 1)}
    r = V.mano_two_hands_shaded_renderer(right_faces=mano['right'].get_faces(), dense_color=np.zeros((778, 3)), img_size=S, device='cuda')
    frames = dev(np.random.default_rng(5).integers(0, 256, (n, S, S, 3)).astype(np.uint8))
    over = V.overlay_predictions(outs, frames, r)
    scale, trans, cl, cr = V.prediction_camera(outs)
    assert torch.equal(scale, s_l / 2) and torch.equal(trans, t_l) and torch.equal(cl, vl)
    cv = torch.cat((cl, cr), 1).contiguous()
    o = V.rasterize_shaded(cv, r.faces, S, colors=r.rgb_coor.flip(-1).contiguous(), scale=scale, trans2d=trans, background=frames,
                           outputs=('pix_to_face', 'bary', 'overlay_u8'))
    torch.cuda.synchronize()
    assert torch.equal(over, o['overlay_u8']) and over.dtype == torch.uint8 and over.shape == (n, S, S, 3)
    both_hands_in_view(o['pix_to_face'])
    p2f, ba, f = o['pix_to_face'].cpu().numpy(), o['bary'].cpu().numpy().astype(np.float64), r.faces.cpu().numpy()
    uv = np.concatenate([(s_l[:, None, None] * vl[..., :2] + t_l[:, None]).cpu().numpy(), (s_r[:, None, None] * vr[..., :2] + t_r[:, None]).cpu().numpy()], 1).astype(np.float64)
    cols, rows = np.meshgrid(np.arange(S), np.arange(S))
    centre = np.stack([(cols + 0.5) * 2 / S - 1, (rows + 0.5) * 2 / S - 1], -1)
    tols = []
    for b in range(n):
        fg = p2f[b] >= 0
        vi = f[np.where(fg, p2f[b], 0)]
        got = (ba[b][..., None] * uv[b][vi]).sum(-2)
        x, y, _ = SH.project_ortho(cv[b].cpu().numpy(), scale[b].item(), trans[b].cpu().numpy())
        area = np.abs(R.edge(x[f[:, 0]], y[f[:, 0]], x[f[:, 1]], y[f[:, 1]], x[f[:, 2]], y[f[:, 2]])).astype(np.float64)
        tol = 1e-5 + 2e-8 / area[np.where(fg, p2f[b], 0)]
        err = np.abs(got - centre).max(-1)
        assert (err[fg] <= tol[fg]).all(), (b, float((err - tol)[fg].max()))
        tols.append(tol[fg])
    assert np.median(np.concatenate(tols)) < 2e-4                         # the bound bites: a wrong sign, factor or translation costs 1e-2 and more
    # the frames show through outside the hands
    bgm = (p2f < 0)
    assert np.array_equal(over.cpu().numpy()[bgm], frames.cpu().numpy()[bgm])


def test_draw_joints_matches_its_restatement():
    S, B = 256, 3
    rng = np.random.default_rng(11)
    img = rng.integers(0, 256, (B, S, S, 3)).astype(np.uint8)
    uv = rng.uniform(-0.9, 0.9, (2, B, 21, 2)).astype(np.float32)
    uv[0, 0, 5] = uv[0, 0, 6]                                             # a zero-length bone
    uv[1, 1, 3] = [1.4, -1.2]                                             # a joint outside the picture
    uv[0, 2, 2] = [(2 * 100 + 1) / S - 1, (2 * 50 + 1) / S - 1]            # exactly on a pixel centre
    got = V.draw_joints(dev(img), dev(uv[0]), dev(uv[1]))
    torch.cuda.synchronize()
    for b in range(B):
        want = SH.draw_joints(img[b], uv[0, b], uv[1, b], V.JOINT_PALETTE)
        assert np.array_equal(got[b].cpu().numpy(), want), b
        assert 0.005 < (want != img[b]).any(-1).mean() < 0.5
    L, P = _capi.lib(), _capi.ptr
    g, u = dev(img), dev(uv[0])
    assert L.dir_render_joints(None, P(u), P(u), B, S, 3.0, 1.0, None) < 0
    assert L.dir_render_joints(P(g), P(u), P(u), B, 8, 3.0, 1.0, None) < 0
    assert L.dir_render_joints(P(g), P(u), P(u), B, S, -1.0, 1.0, None) < 0
    assert L.dir_render_joints(P(g), P(u), P(u), 0, S, 3.0, 1.0, None) == 0


def test_visualize_command(tmp_path, state, mano, capsys):
    """python -m dir_amd.apps.visualize on the fake split with synthetic weights: one PNG per requested index; its left half is the decoded
    frame, its right half overlay_predictions of the same batch, byte for byte"""
    from PIL import Image

    from dir_amd.apps import visualize as VZ
    from dir_amd.engine import DirEngine
    n, bs = 5, 2
    root, out = str(tmp_path / 'data'), str(tmp_path / 'pics')
    write_split(root, 7, seed=3)
    ck = str(tmp_path / 'DIR.pth')
    torch.save({'net': state}, ck)
    assert VZ.main(['--model', ck, '--data_path', root, '--out', out, '--num', str(n), '--bs', str(bs), '--workers', '2']) == n
    assert 'images/s' in capsys.readouterr().out
    assert sorted(os.listdir(out)) == sorted('%d.png' % i for i in range(n))
    ds = DS.InterHandSplit(root)
    eng = DirEngine(state, dtype=torch.float16)
    r = V.mano_two_hands_shaded_renderer(right_faces=mano['right'].get_faces(), dense_color=np.zeros((778, 3)), img_size=256, device='cuda')
    covered = 0
    for b0 in range(0, n, bs):
        idx = list(range(b0, min(n, b0 + bs)))
        frames = dev(np.stack([ds.frame(i) for i in idx]))
        outs = eng.forward(frames, want_proj_feat=False)
        over = V.overlay_predictions(outs[2], frames, r).cpu().numpy()
        for j, i in enumerate(idx):
            with Image.open(os.path.join(out, '%d.png' % i)) as im:
                pic = np.asarray(im.convert('RGB'))[:, :, ::-1]
            assert pic.shape == (256, 512, 3)
            assert np.array_equal(pic[:, :256], frames[j].cpu().numpy()), i
            assert np.array_equal(pic[:, 256:], over[j]), i
            covered += int((pic[:, 256:] != pic[:, :256]).any(-1).sum())
    # --joints draws on top of the same overlay
    out2 = str(tmp_path / 'pics_joints')
    assert VZ.main(['--model', ck, '--data_path', root, '--out', out2, '--num', '2', '--bs', '2', '--workers', '2', '--joints', '--stage', '1']) == 2
    frames = dev(np.stack([ds.frame(i) for i in range(2)]))
    outs = eng.forward(frames, want_proj_feat=False)
    over = V.draw_joints(V.overlay_predictions(outs[1], frames, r), outs[1]['pd_joint_uv_left'], outs[1]['pd_joint_uv_right']).cpu().numpy()
    for i in range(2):
        with Image.open(os.path.join(out2, '%d.png' % i)) as im:
            assert np.array_equal(np.asarray(im.convert('RGB'))[:, 256:, ::-1], over[i]), i
