"""CPU-only: the numpy restatement of the shaded / orthographic renderer (tests/helpers/shade_ref.py) against closed forms, so that it
is not merely a copy of the kernel's thinking, and the parts of the new interface that need no device.

Tolerance of (a)-(d): chains of a few dozen float32 roundings on values of order 1, so 1e-5 absolute."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'helpers'))
import raster_ref as R  # noqa: E402
import shade_ref as SH  # noqa: E402

TOL = 1e-5


def icosahedron():
    t = (1 + 5 ** 0.5) / 2
    v = np.array([(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t),
                  (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)], np.float64)
    f = np.array([(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
                  (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)])
    return v, f


def test_a_icosahedron_normals_are_the_normalised_positions():
    v, f = icosahedron()
    for radius in (1.0, 0.37):
        vv = (v / np.linalg.norm(v, axis=1, keepdims=True) * radius).astype(np.float32)
        n = SH.vertex_normals(vv, f)
        want = v / np.linalg.norm(v, axis=1, keepdims=True)
        assert n.dtype == np.float32 and np.abs(n - want).max() < TOL
    # the other winding turns every normal round; a vertex of no face keeps a zero normal; an index outside the table adds nothing
    assert np.abs(SH.vertex_normals(vv, f[:, [1, 0, 2]]) + want).max() < TOL
    extra = np.concatenate([vv, [[5.0, 5.0, 5.0]]]).astype(np.float32)
    n = SH.vertex_normals(extra, np.concatenate([f, [[0, 1, 13], [-1, 2, 3]]]))
    assert np.array_equal(n[12], np.zeros(3, np.float32)) and np.abs(n[:12] - want).max() < TOL


def lit_square():
    """a square in the plane z = 0, wound so that its normals are (0, 0, -1): towards the light at (0, 0, -1) and the camera"""
    v = np.array([(-0.5, -0.5, 0), (-0.5, 0.5, 0), (0.5, 0.5, 0), (0.5, -0.5, 0)], np.float32)
    f = np.array([(0, 1, 2), (0, 2, 3)])
    return v, f


def square_closed_form(x, y, col):
    """float64: the colour at the world point (x, y, 0) of the square under the reference light and the orthographic camera"""
    l = np.sqrt(x * x + y * y + 1.0)                                      # |location - p|
    c = 1.0 / l                                                           # n . d with n = (0, 0, -1)
    vw = np.sqrt(x * x + y * y + 100.0)                                   # |centre - p|, centre (0, 0, -10)
    a = np.maximum((10.0 - x * x - y * y) / (l * vw), 0.0)                # view . r with r = (x, y, -1) / l
    return (0.5 + 0.3 * c)[..., None] * np.asarray(col, np.float64) + 0.2 * (a ** 64)[..., None]


def test_b_lit_square_matches_the_closed_form():
    v, f = lit_square()
    n = SH.vertex_normals(v, f)
    assert np.array_equal(n, np.tile(np.array([0, 0, -1], np.float32), (4, 1)))
    col = np.array([204.0, 153.0, 0.0])
    colors = np.tile(col.astype(np.float32), (4, 1))
    # straight under the light (no pixel centre lies there when S is even): p = (v0 + v2) / 2 = 0, colour = 0.8 c + 0.2
    under = SH.phong(np.zeros((1, 1), np.int32), np.array([[[0.5, 0.0, 0.5]]], np.float32), f, v, n, colors, SH.POINT_LIGHT, (0, 0, -10))
    assert np.abs(under[0, 0] - (0.8 * col + 0.2)).max() < TOL * 255
    assert np.abs(square_closed_form(np.zeros(1), np.zeros(1), col)[0] - (0.8 * col + 0.2)).max() < 1e-12
    S = 64
    out = SH.render(v, f, S, colors, scale=0.5, trans2d=(0.0, 0.0))       # focal 1: x_ndc = -x
    fg = out['pix_to_face'] >= 0
    # the middle half of each axis, less the pixel centres on the shared diagonal: coverage is strict, so neither triangle takes them
    assert fg.sum() == (S // 2) ** 2 - S // 2 and not fg[np.arange(S), np.arange(S)].any()
    rows, cols = np.nonzero(fg)
    x, y = (2 * cols + 1) / S - 1.0, (2 * rows + 1) / S - 1.0             # x_ndc = 1 - (2c+1)/S = -x
    want = square_closed_form(x, y, col) / 255.0
    assert np.abs(out['shaded_f32'][rows, cols] - want).max() < TOL
    assert np.all(out['shaded_f32'][~fg] == np.float32(1) / np.float32(255))
    assert np.allclose(out['zbuf'][fg], 10.0, atol=TOL) and np.all(out['zbuf'][~fg] == -1)
    # the overlay: the frame's bytes outside, the rounded colour inside
    frame = np.random.default_rng(0).integers(0, 256, (S, S, 3)).astype(np.uint8)
    ov = SH.render(v, f, S, colors, scale=0.5, trans2d=(0.0, 0.0), background=frame)['overlay_u8']
    assert np.array_equal(ov[~fg], frame[~fg])
    assert np.abs(ov[rows, cols].astype(np.float64) - want * 255).max() <= 0.5 + TOL * 255


def two_patch_scene(seed, scale, trans2d, nx=26, ny=29):
    """two jittered grid patches ('hands') of nx x ny vertices, left under right in the face table as in the two-hand mesh, placed through
    the inverse of the orthographic camera so that they overlap in the middle of the image; no near-degenerate faces"""
    rng = np.random.default_rng(seed)
    verts, faces = [], []
    for h, (cx, cy) in enumerate(((-0.2, -0.1), (0.2, 0.15))):
        gx, gy = np.meshgrid(np.linspace(-0.35, 0.35, nx), np.linspace(-0.35, 0.35, ny))
        uv = np.stack([gx + cx, gy + cy], -1).reshape(-1, 2) + rng.uniform(-0.002, 0.002, (nx * ny, 2))
        xy = (uv - np.asarray(trans2d)) / (2 * scale)
        z = rng.uniform(-0.1, 0.1, (nx * ny, 1)) + 0.05 * h
        verts.append(np.concatenate([xy, z], -1))
        i = (np.arange(ny - 1)[:, None] * nx + np.arange(nx - 1)[None, :]).reshape(-1) + h * nx * ny
        faces.append(np.concatenate([np.stack([i, i + 1, i + nx], -1), np.stack([i + 1, i + nx + 1, i + nx], -1)]))
    return np.concatenate(verts).astype(np.float32), np.concatenate(faces), len(faces[0])


def test_c_every_covered_pixel_reconstructs_its_centre():
    S, scale, trans2d = 128, 0.8, (0.1, -0.05)
    v, f, n_left = two_patch_scene(1, scale, trans2d, nx=10, ny=11)
    x, y, _ = SH.project_ortho(v, scale, trans2d)
    area = np.abs(R.edge(x[f[:, 0]], y[f[:, 0]], x[f[:, 1]], y[f[:, 1]], x[f[:, 2]], y[f[:, 2]]))
    # b_i = e_i / (area + 1e-8) scales the reconstructed centre by area / (area + 1e-8): with |centre| < 1 that costs up to 1e-8 / area,
    # so the faces are kept above 2e-3 (edge-function units, twice the triangle's area), which leaves 5e-6 to the roundings
    assert area.min() > 2e-3
    p2f, zb, ba = SH.rasterize_ortho(v, f, scale, trans2d, S)
    fg = p2f >= 0
    assert ((p2f >= 0) & (p2f < n_left)).mean() > 0.02 and (p2f >= n_left).mean() > 0.02       # not vacuous: both hands are in view
    uv = 2 * scale * v[:, :2].astype(np.float64) + np.asarray(trans2d)   # DIR's projection with s = 2 scale
    vi = f[np.where(fg, p2f, 0)]
    got = (ba.astype(np.float64)[..., None] * uv[vi]).sum(-2)
    cols, rows = np.meshgrid(np.arange(S), np.arange(S))
    want = np.stack([(cols + 0.5) * 2 / S - 1, (rows + 0.5) * 2 / S - 1], -1)
    assert np.abs(got - want)[fg].max() < TOL                             # every covered pixel, none left out
    assert np.abs(ba[fg].sum(-1) - 1).max() < TOL and np.all(zb[fg] > 9) and np.all(zb[~fg] == -1)
    # the nearer patch wins where they overlap: zbuf is the smallest depth of any covering face (checked through the depth itself)
    depth = (ba.astype(np.float64) * (v[:, 2].astype(np.float64) + 10)[vi]).sum(-1)
    assert np.abs(depth - zb)[fg].max() < TOL


def test_d_right_hand_remap_gives_the_right_cameras_uv():
    rng = np.random.default_rng(2)
    for _ in range(20):
        sl, sr = rng.uniform(0.3, 3.0, 2)
        tl, tr = rng.uniform(-1, 1, (2, 2))
        vr = rng.uniform(-0.2, 0.2, (50, 3))
        moved = SH.remap_right_hand(sl, tl, sr, tr, vr)
        assert np.abs((2 * sl * moved[:, :2] + tl) - (2 * sr * vr[:, :2] + tr)).max() < TOL
        assert np.abs(moved[:, 2] - sr / sl * vr[:, 2]).max() < TOL     # the depth is scaled with the rest (vis_utils.py:321)


def test_e_ambient_light_is_the_plain_texel_bit_for_bit():
    S, scale, trans2d = 64, 0.8, (0.1, -0.05)
    v, f, _ = two_patch_scene(3, scale, trans2d, nx=12, ny=13)
    colors = (np.random.default_rng(4).random((len(v), 3)) * 255).astype(np.float32)
    out = SH.render(v, f, S, colors, scale=scale, trans2d=trans2d, lights=SH.AMBIENT_LIGHT)
    want = R.texel(out['pix_to_face'], out['bary'], f, colors) / np.float32(255)
    assert (out['pix_to_face'] >= 0).mean() > 0.1
    assert np.array_equal(out['shaded_f32'].view(np.uint32), want.view(np.uint32))
    # and under the perspective camera, where the rasteriser is raster_ref's own
    K = np.array([[-S / 2, 0, S / 2], [0, -S / 2, S / 2], [0, 0, 1]], np.float32)       # x_ndc = X / Z
    vp = v.copy()
    vp[:, 2] += 0.6
    out = SH.render(vp, f, S, colors, K=K, lights=SH.AMBIENT_LIGHT)
    p2f, zb, ba = R.rasterize(vp, f, K, S)
    assert np.array_equal(out['pix_to_face'], p2f) and np.array_equal(out['bary'].view(np.uint32), ba.view(np.uint32))
    assert (p2f >= 0).mean() > 0.05
    assert np.array_equal(out['shaded_f32'].view(np.uint32), (R.texel(p2f, ba, f, colors) / np.float32(255)).view(np.uint32))
    # the point light changes the picture
    lit = SH.render(vp, f, S, colors, K=K)['shaded_f32']
    assert np.abs(lit - out['shaded_f32'])[p2f >= 0].max() > 0.05


def test_f_import_and_base_class():
    from dir_amd.utils import vis_utils as V
    from dir_amd.utils.vis_utils import mano_two_hands_shaded_renderer, overlay_predictions, rasterize_shaded, vertex_normals
    assert callable(rasterize_shaded) and callable(vertex_normals) and callable(overlay_predictions)
    base, sub = V.mano_two_hands_renderer, mano_two_hands_shaded_renderer
    assert issubclass(sub, base)
    for name in ('render_rgb', 'render_rgb_orth', '_raster'):
        assert name in sub.__dict__ and getattr(sub, name) is not getattr(base, name)
    for name in ('render_mask', 'render_densepose', 'render_depth'):
        assert name not in sub.__dict__                                   # inherited: they reach the orthographic camera through _raster
    # the base class still lacks them (no device object is made: the refusals come before anything is touched)
    with pytest.raises(NotImplementedError):
        base.render_rgb(object(), cameras=None)
    with pytest.raises(NotImplementedError):
        base.render_rgb_orth(object())
    with pytest.raises(NotImplementedError):
        base._raster(object(), None, 1.0, 1.0, None, None, None, ('zbuf',))
    # argument rules that need no device
    import torch
    z = torch.zeros(1, V.NV, 3)
    with pytest.raises(ValueError, match='exactly one camera'):
        rasterize_shaded(z, None, 64, K=torch.zeros(1, 3, 3), scale=torch.ones(1), trans2d=torch.zeros(1, 2))
    with pytest.raises(ValueError, match='exactly one camera'):
        rasterize_shaded(z, None, 64)
    with pytest.raises(ValueError, match='both scale'):
        rasterize_shaded(z, None, 64, scale=torch.ones(1))
    with pytest.raises(ValueError):
        V.Lights(0.5, 0.3, 0.2, shininess=32)
    assert V.POINT_LIGHT.ambient == (0.5,) * 3 and V.POINT_LIGHT.diffuse == (0.3,) * 3 and V.POINT_LIGHT.specular == (0.2,) * 3
    assert V.POINT_LIGHT.location == (0.0, 0.0, -1.0)
    c = V.default_colors()
    assert c.shape == (V.NV, 3) and tuple(c[0]) == (204, 153, 0) and tuple(c[-1]) == (102, 102, 255)


def test_c_abi_refuses_bad_arguments_before_any_launch():
    """dir_render_shaded / dir_render_vertex_normals / dir_render_adjacency: every argument check fails with a negative code and a message
    on the host, so this runs without a device (the pointers are never dereferenced)"""
    import torch  # noqa: F401
    from dir_amd import _capi
    L = _capi.lib()
    one = ctypes.c_void_p(256)
    lights = _capi.RenderLights((ctypes.c_float * 3)(0.5, 0.5, 0.5), (ctypes.c_float * 3)(0.3, 0.3, 0.3), (ctypes.c_float * 3)(0.2, 0.2, 0.2),
                                (ctypes.c_float * 3)(0, 0, -1), 64.0)
    B, S = 2, 64
    ws = int(L.dir_render_shaded_workspace_bytes(B))
    assert ws == B * (3076 * 4 + 1556 * 3 * 4) and L.dir_render_shaded_workspace_bytes(0) == 0
    assert L.dir_render_adjacency_bytes() == (1556 + 1 + 3 * 3076) * 4
    # verts faces adjacency K scale trans2d colors lights background B S workspace bytes p2f zbuf bary shaded overlay stream
    ok = [one, one, one, None, one, one, one, lights, None, B, S, one, ws, None, None, None, one, None, None]

    def bad(args, word):
        rc = L.dir_render_shaded(*args)
        assert rc < 0 and word in L.dir_last_error(), (rc, L.dir_last_error())

    def changed(**kw):
        names = ('verts', 'faces', 'adjacency', 'K', 'scale', 'trans2d', 'colors', 'lights', 'background', 'B', 'S', 'workspace', 'bytes',
                 'p2f', 'zbuf', 'bary', 'shaded', 'overlay', 'stream')
        a = list(ok)
        for k, v in kw.items():
            a[names.index(k)] = v
        return a
    bad(changed(K=one), b'both given')
    bad(changed(scale=None, trans2d=None), b'none given')
    bad(changed(trans2d=None), b'both scale and trans2d')
    bad(changed(verts=None), b'null pointer')
    bad(changed(faces=None), b'null pointer')
    bad(changed(workspace=None), b'null pointer')
    bad(changed(S=15), b'outside 16..1024')
    bad(changed(S=1025), b'outside 16..1024')
    bad(changed(B=-1), b'outside 1..')
    bad(changed(bytes=ws - 1), b'needed')
    bad(changed(colors=None), b'colour output needs')
    bad(changed(adjacency=None), b'colour output needs')
    bad(changed(lights=None), b'colour output needs')
    bad(changed(shaded=None), b'no output')
    bad(changed(background=one), b'overlay_u8 only')
    dim = _capi.RenderLights((ctypes.c_float * 3)(1, 1, 1), (ctypes.c_float * 3)(), (ctypes.c_float * 3)(), (ctypes.c_float * 3)(), 32.0)
    bad(changed(lights=dim), b'only 64')
    assert L.dir_render_shaded(*changed(B=0, verts=None, workspace=None, bytes=0)) == 0        # an empty batch is a no-op
    assert L.dir_render_vertex_normals(None, one, one, B, one, None) < 0 and b'null pointer' in L.dir_last_error()
    assert L.dir_render_vertex_normals(one, one, None, B, one, None) < 0
    assert L.dir_render_vertex_normals(None, None, None, 0, None, None) == 0
    assert L.dir_render_adjacency(None, one, 1 << 20, None) < 0
    assert L.dir_render_adjacency(one, one, 16, None) < 0 and b'needed' in L.dir_last_error()
