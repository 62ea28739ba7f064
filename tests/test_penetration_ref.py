"""CPU-only: the float64 restatement of the penetration measures (tests/helpers/penetration_ref.py) against closed forms, the host
helper close_boundary, and the host-side contract of the two C entry points (no launch: there is no GPU here)."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'helpers'))
import penetration_ref as R  # noqa: E402

from test_capi_exports import declared_symbols  # noqa: E402


def test_winding_number_of_a_sphere_is_one_inside_and_zero_outside():
    v, f = R.octasphere(3)
    assert v.shape == (258, 3) and f.shape == (512, 3)
    g = np.random.default_rng(0)
    d = g.normal(size=(200, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    inside = d * g.uniform(0, 0.9, (200, 1))               # the inscribed polyhedron holds the ball of radius cos(11.25 deg) > 0.98
    outside = d * g.uniform(1.01, 5, (200, 1))
    assert np.abs(R.winding(inside, v, f) - 1).max() < 1e-12
    assert np.abs(R.winding(outside, v, f)).max() < 1e-12
    assert np.abs(R.winding(inside, v, f[:, [1, 0, 2]]) + 1).max() < 1e-12         # flipped faces: -1, the same |w|


def test_skipped_faces_change_nothing():
    v, f = R.octasphere(2)
    junk = np.array([[0, 0, 1], [3, 5, 3], [7, 7, 7], [0, 1, len(v)], [-1, 2, 3]], np.int32)
    f2 = np.concatenate([f[:10], junk, f[10:]])
    assert len(R.valid_faces(f2, len(v))) == len(f)
    p = np.random.default_rng(1).uniform(-1.5, 1.5, (50, 3))
    assert np.array_equal(R.winding(p, v, f2), R.winding(p, v, f)) and np.array_equal(R.distance(p, v, f2), R.distance(p, v, f))
    assert np.isfinite(R.distance(p, v, f2)).all()


def test_distance_to_a_cube_is_the_closed_form():
    v, f = R.cube(0.5, (0.1, -0.2, 0.3))
    g = np.random.default_rng(2)
    p = g.uniform(-1.5, 1.5, (2000, 3))
    p[:8] = v                                                # the corners themselves: distance 0
    p[8:11] = [[0.1, -0.2, 0.3], [0.6, -0.2, 0.3], [0.1, 0.3, 2.0]]        # the centre, a point on a face, a point above a face
    want = R.cube_distance(p, 0.5, (0.1, -0.2, 0.3))
    assert np.abs(R.distance(p, v, f) - want).max() < 1e-14
    q = p[11:]                                               # (on the surface itself the winding number is not an integer)
    assert np.array_equal(np.abs(R.winding(q, v, f)) > 0.5, (np.abs(q - [0.1, -0.2, 0.3]) < 0.5).all(1)) and (np.abs(R.winding(q, v, f)) > 0.5).sum() > 50


def test_lattice_count_of_two_cubes_is_exact():
    a, fa = R.cube(0.0325)
    b, fb = R.cube(0.0325, (0.03, 0, 0))
    r = R.intersection(a, fa, b, fb, h=0.005)
    assert r['cells'] == 7 * 13 * 13 == 1183 and r['n_both'] == 1183
    assert abs(r['volume'] - 1183 * 0.005 ** 3) < 1e-18
    # no lattice point lies on a face of either cube: the count does not hang on a rounding
    p = r['points'].astype(np.float64)
    gap = min(np.abs(np.abs(p) - 0.0325).min(), np.abs(np.abs(p - [0.03, 0, 0]) - 0.0325).min())
    assert gap > 0.002
    assert np.abs(np.abs(r['w_a']) - 1).max() < 1e-12 and np.abs(np.abs(r['w_b']) - 1).max() < 1e-12
    over = R.intersection(a, fa, b, fb, h=0.005, max_cells=1182)
    assert over['cells'] == 1183 and over['n_both'] == 0 and np.isnan(over['volume'])


LENS_R, LENS_D = 0.03, 0.03


def test_lens_volume_of_two_spheres():
    """Two spheres of radius 30 mm, centres 30 mm apart, subdivision 4 (1 026 vertices, 2 048 faces), 5 mm lattice, against the lens
    formula pi (4R + d) (2R - d)^2 / 12 = 35.34 cm^3.  Measured: 35.000 cm^3 (280 lattice points), 0.97 % below the formula -- the
    inscribed polyhedra are smaller than the spheres and the 5 mm voxels quantise the rest.  Gate: 1.5 x the measured error = 1.46 %."""
    a, fa = R.octasphere(4, LENS_R, (0.001, 0.002, 0.0005))          # off the lattice, so that no point sits on the symmetry planes
    b, fb = R.octasphere(4, LENS_R, (0.001 + LENS_D, 0.002, 0.0005))
    r = R.intersection(a, fa, b, fb, h=0.005)
    exact = np.pi * (4 * LENS_R + LENS_D) * (2 * LENS_R - LENS_D) ** 2 / 12
    err = abs(r['volume'] - exact) / exact
    print('lens: %d lattice points, %.3f cm^3 against %.3f cm^3, relative error %.4f' % (r['n_both'], r['volume'] * 1e6, exact * 1e6, err))
    assert err < 0.0146


def test_penetration_of_two_spheres():
    """sphere B (radius 1) centred 1.5 from sphere A (radius 1): A's vertices inside B are those within 1 of B's centre; the deepest
    is A's pole facing B, 0.5 under B's surface (to the faceting: the polyhedron lies up to 1 - cos(5.6 deg) = 0.005 inside the sphere)"""
    a, fa = R.octasphere(3)
    b, fb = R.octasphere(3, 1.0, (1.5, 0, 0))
    r = R.penetration(a, fa, b, fb)
    want = (np.linalg.norm(a - [1.5, 0, 0], axis=1) < 0.99).sum()
    assert r['count'][0] == r['count'][1] == want > 10
    assert 0.49 < r['max_depth'][0] <= 0.5 and abs(r['max_depth'][0] - r['max_depth'][1]) < 1e-12 and r['depth'] == r['max_depth'].max()
    far = R.penetration(a, fa, b + [3, 0, 0], fb)
    assert far['count'].sum() == 0 and far['depth'] == 0 and far['sum_depth'].sum() == 0


def _edge_directions(f):
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    seen = {}
    for u, v in e:
        seen.setdefault((min(u, v), max(u, v)), []).append(u < v)
    return seen


@pytest.mark.parametrize('mesh', ['hemisphere', 'cylinder', 'cylinder_flipped'])
def test_close_boundary_seals_a_single_loop(mesh):
    from dir_amd.utils.penetration import close_boundary
    v, f = R.open_hemisphere(3) if mesh == 'hemisphere' else R.open_cylinder(24)
    if mesh == 'cylinder_flipped':
        f = np.ascontiguousarray(f[:, [1, 0, 2]])
    inner = np.array([[0.1, -0.2, 0.4]])
    assert abs(abs(R.winding(inner, v, f)[0]) - 1) > 1e-3                     # open: not an integer
    assert any(len(d) == 1 for d in _edge_directions(f).values())
    g = close_boundary(f)
    assert g.dtype == np.int32 and np.array_equal(g[:len(f)], f) and g.max() < len(v)
    loop = sum(len(d) == 1 for d in _edge_directions(f).values())
    assert len(g) == len(f) + loop - 2                                       # a fan over the loop, no new vertex
    assert all(len(d) == 2 and d[0] != d[1] for d in _edge_directions(g).values())      # every edge: two faces, opposite directions
    assert abs(abs(R.winding(inner, v, g)[0]) - 1) < 1e-12
    assert abs(R.winding(np.array([[0.1, -0.2, -0.4]]), v, g)[0]) < 1e-12


def test_close_boundary_rejects_what_is_not_one_loop():
    from dir_amd import synth
    from dir_amd.utils.penetration import close_boundary
    with pytest.raises(ValueError):
        close_boundary(np.asarray(synth.synthetic_mano_tables('right')['f']).astype(np.int64))       # a triangle soup
    v, f = R.octasphere(1)
    with pytest.raises(ValueError):
        close_boundary(f)                                                      # closed: no boundary
    with pytest.raises(ValueError):
        close_boundary(np.delete(f, [0, len(f) - 1], 0))                       # two holes
    with pytest.raises(ValueError):
        close_boundary(np.zeros((4, 2), np.int32))


def test_binding_covers_the_header_and_versions_agree():
    from dir_amd import _capi
    syms = declared_symbols()
    assert 'dir_mesh_penetration' in syms and 'dir_mesh_intersection_volume' in syms
    assert sorted(_capi._SIGNATURES) == syms


def test_entry_points_reject_bad_arguments_before_any_launch():
    import torch  # noqa: F401
    from dir_amd import _capi, build
    build.build(verbose=False)
    L = _capi.lib()
    assert L.dir_abi_version() == _capi.ABI_VERSION
    one = ctypes.c_void_p(16)

    def bad(rc, word):
        assert rc != 0 and word in L.dir_last_error(), (rc, L.dir_last_error())

    def pen(va=one, fa=one, vb=one, fb=one, B=2, Va=778, Fa=1538, Vb=778, Fb=1538, cnt=one, mx=one, sm=one):
        return L.dir_mesh_penetration(va, fa, vb, fb, B, Va, Fa, Vb, Fb, None, None, cnt, mx, sm, None)

    def vol(va=one, fa=one, vb=one, fb=one, B=2, Va=778, Fa=1538, Vb=778, Fb=1538, h=0.005, cells=1 << 17, v=one, nb=one, nc=one):
        return L.dir_mesh_intersection_volume(va, fa, vb, fb, B, Va, Fa, Vb, Fb, h, cells, v, nb, nc, None)
    for call in (pen, vol):
        for k in ('va', 'fa', 'vb', 'fb'):
            bad(call(**{k: None}), b'null pointer')
        bad(call(B=0), b'batch')
        bad(call(B=-3), b'batch')
        bad(call(Va=4097), b'vertices')
        bad(call(Vb=0), b'vertices')
        bad(call(Fa=8193), b'faces')
        bad(call(Fb=0), b'faces')
    for k in ('cnt', 'mx', 'sm'):
        bad(pen(**{k: None}), b'null pointer')
    for k in ('v', 'nb', 'nc'):
        bad(vol(**{k: None}), b'null pointer')
    bad(vol(h=0.0), b'pitch')
    bad(vol(h=-0.005), b'pitch')
    bad(vol(h=float('nan')), b'pitch')
    bad(vol(h=float('inf')), b'pitch')
    bad(vol(cells=0), b'max_cells')
    bad(vol(cells=(1 << 24) + 1), b'max_cells')
