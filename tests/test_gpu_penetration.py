"""GPU: dir_mesh_penetration / dir_mesh_intersection_volume (csrc/penetration.hip) held to the float64 numpy restatement
tests/helpers/penetration_ref.py, which tests/test_penetration_ref.py checks against closed forms; then the wiring into apps.eval and
apps.train.validate.

Inputs: closed meshes (two octahedron spheres of 30 mm radius 30 mm apart at subdivision 3 and 4 -- the latter takes two LDS chunks of
faces and two query vertices per thread --, two 65 mm cubes) and six pairs from the synthetic MANO table (the right template and its
mirror, per-vertex noise 3 mm, relative offset 20 mm, seed 0: triangle soups whose winding numbers range over -14 .. 10), each pair
alone (B = 1) and as a row of a B = 64 batch.

Measured on the MI355X, largest absolute error of the kernels against the restatement over all of these inputs:
    winding  8.25e-5      distance  7.9e-9 m
(both set by the synthetic pairs; numpy's own float32 evaluation of the same formulas gives 8.2e-5 and 6.3e-9 m there: one vertex 2 nm
from a triangle sets the winding figure).  The gates are 4 x the measured values, for float32 sums taken in another order: 3.3e-4 and
3.2e-8 m, under the issue's caps of 5e-4 and 1e-6 m.  The inside masks and the lattice counts must equal
the restatement's except at points whose float64 ||w| - 0.5| is below BAND = the winding gate; at most 1 % of any test's points may
be left out that way."""
import json
import os
import shutil
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'helpers'))
import penetration_ref as R  # noqa: E402
from fake_split import write_split  # noqa: E402

from dir_amd import synth  # noqa: E402
from dir_amd.utils import penetration as PN  # noqa: E402

pytestmark = pytest.mark.gpu

WIND_MEASURED, DIST_MEASURED = 8.25e-5, 7.9e-9
WIND_GATE, DIST_GATE = min(4 * WIND_MEASURED, 5e-4), min(4 * DIST_MEASURED, 1e-6)
BAND = WIND_GATE
ROWS = (0, 7, 21, 38, 50, 63)            # where the six reference pairs sit in the B = 64 batch
PITCH = 0.005


def dev(x, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dtype).cuda()


def run_pen(a, fa, b, fb, per_vertex=True):
    out = PN.mesh_penetration(dev(a), dev(fa, torch.int32), dev(b), dev(fb, torch.int32), per_vertex=per_vertex)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def run_vol(a, fa, b, fb, pitch=PITCH, max_cells=1 << 17):
    out = PN.intersection_volume(dev(a), dev(fa, torch.int32), dev(b), dev(fb, torch.int32), pitch=pitch, max_cells=max_cells)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def closed_cases():
    """name -> (verts_a [1,V,3] float32, faces_a, verts_b, faces_b)"""
    f32 = lambda v: v.astype(np.float32)[None]  # noqa: E731
    cases = {}
    for sub in (3, 4):
        a, fa = R.octasphere(sub, 0.03, (0.001, 0.002, 0.0005))
        b, fb = R.octasphere(sub, 0.03, (0.031, 0.002, 0.0005))
        cases['spheres%d' % sub] = (f32(a), fa, f32(b), fb)
    a, fa = R.cube(0.0325)
    b, fb = R.cube(0.0325, (0.03, 0.01, -0.02))
    cases['cubes'] = (f32(a), fa, f32(b), fb[:, [1, 0, 2]])           # B inside out: |w| does not care
    return cases


@pytest.fixture(scope='module')
def pairs():
    return R.hand_pairs(6, seed=0)


@pytest.fixture(scope='module')
def batch64(pairs):
    a, fa, b, fb = R.hand_pairs(64, seed=1)
    for k, r in enumerate(ROWS):
        a[r], b[r] = pairs[0][k], pairs[2][k]
    return a, fa, b, fb


@pytest.fixture(scope='module')
def pair_refs(pairs):
    a, fa, b, fb = pairs
    return [R.penetration(a[k], fa, b[k], fb) for k in range(len(a))]


@pytest.fixture(scope='module')
def lattice_refs(pairs):
    a, fa, b, fb = pairs
    return [R.intersection(a[k], fa, b[k], fb, PITCH) for k in range(len(a))]


def check_against(ref, got, row, n_a, what):
    """one sample of the kernel's output against the restatement's dict -> (winding error, distance error)"""
    w, d = got['winding'][row].astype(np.float64), got['dist'][row].astype(np.float64)
    ew, ed = np.abs(w - ref['winding']).max(), np.abs(d - ref['dist']).max()
    print('%s: max |winding - ref| = %.3e, max |dist - ref| = %.3e m' % (what, ew, ed))
    near = np.abs(np.abs(ref['winding']) - 0.5) < BAND
    print('%s: %d of %d vertices within %.1e of the threshold' % (what, near.sum(), near.size, BAND))
    assert near.sum() <= 0.01 * near.size, what
    inside, inside_ref = np.abs(w) > 0.5, np.abs(ref['winding']) > 0.5
    assert np.array_equal(inside[~near], inside_ref[~near]), what
    if not near.any():
        assert np.array_equal(got['count'][row], ref['count']), what
    return ew, ed


def check_aggregates(got, n_a, what):
    """count / max_depth equal numpy on the kernel's own per-vertex outputs exactly, sum_depth to 1e-6 relative"""
    for row in range(len(got['count'])):
        own = R.aggregate(got['winding'][row], got['dist'][row], n_a)
        assert np.array_equal(got['count'][row], own['count']), what
        assert np.array_equal(got['max_depth'][row], own['max_depth'].astype(np.float32)), what
        assert np.allclose(got['sum_depth'][row], own['sum_depth'], rtol=1e-6, atol=0), what
        assert got['depth'][row] == got['max_depth'][row].max(), what


def test_per_vertex_outputs_and_aggregates_match_the_restatement(pairs, batch64, pair_refs):
    errs = []
    for name, (a, fa, b, fb) in closed_cases().items():
        got = run_pen(a, fa, b, fb)
        errs.append(check_against(R.penetration(a[0], fa, b[0], fb), got, 0, a.shape[1], name))
        check_aggregates(got, a.shape[1], name)
        assert got['count'][0].min() > 0 and got['depth'][0] > 0.005, name          # these really overlap
    a, fa, b, fb = pairs
    alone = [run_pen(a[k:k + 1], fa, b[k:k + 1], fb) for k in range(len(a))]
    for k, got in enumerate(alone):
        errs.append(check_against(pair_refs[k], got, 0, a.shape[1], 'pair %d alone' % k))
        check_aggregates(got, a.shape[1], 'pair %d alone' % k)
    a64, _, b64, _ = batch64
    got64 = run_pen(a64, fa, b64, fb)
    check_aggregates(got64, a.shape[1], 'B = 64')
    for k, r in enumerate(ROWS):
        errs.append(check_against(pair_refs[k], got64, r, a.shape[1], 'pair %d as row %d of 64' % (k, r)))
        for key in got64:
            assert np.array_equal(got64[key][r], alone[k][key][0]), (key, k)          # bit-identical in any batch
    ew, ed = max(e[0] for e in errs), max(e[1] for e in errs)
    print('MEASURED: winding %.3e (gate %.3e), distance %.3e m (gate %.3e m)' % (ew, WIND_GATE, ed, DIST_GATE))
    assert ew < WIND_GATE and ed < DIST_GATE


def test_outputs_without_the_per_vertex_arrays_are_the_same(pairs):
    a, fa, b, fb = pairs
    full, lean = run_pen(a, fa, b, fb), run_pen(a, fa, b, fb, per_vertex=False)
    assert sorted(lean) == ['count', 'depth', 'max_depth', 'sum_depth']
    assert all(np.array_equal(full[k], lean[k]) for k in lean)


def test_two_runs_and_any_batch_give_identical_bits(batch64):
    a, fa, b, fb = batch64
    p1, p2 = run_pen(a, fa, b, fb), run_pen(a, fa, b, fb)
    v1, v2 = run_vol(a, fa, b, fb), run_vol(a, fa, b, fb)
    for x, y in ((p1, p2), (v1, v2)):
        assert all(np.array_equal(x[k], y[k], equal_nan=True) for k in x)
    for r in (0, 5, 31, 63):
        ps, vs = run_pen(a[r:r + 1], fa, b[r:r + 1], fb), run_vol(a[r:r + 1], fa, b[r:r + 1], fb)
        assert all(np.array_equal(ps[k][0], p1[k][r]) for k in ps), r
        assert all(np.array_equal(vs[k][0], v1[k][r], equal_nan=True) for k in vs), r
    assert (v1['cells'] >= v1['n_both']).all() and (v1['n_both'] > 0).sum() > 32


def test_skipped_faces_are_skipped_on_the_device():
    """the synthetic table has 7 faces with a repeated index; more junk (an index past the end, a negative one) changes nothing"""
    a, fa, b, fb = R.hand_pairs(2, seed=5)
    assert len(R.valid_faces(fb, 778)) == len(fb) - 7
    junk = np.array([[0, 0, 5], [1, 2, 778], [-1, 2, 3], [9, 9, 9]], np.int32)
    fb2, fa2 = np.concatenate([fb[:100], junk, fb[100:]]), np.concatenate([junk, fa])
    x, y = run_pen(a, fa, b, fb), run_pen(a, fa2, b, fb2)
    # the valid faces come in the same order, so the sums are the same bits
    assert all(np.array_equal(x[k], y[k]) for k in x) and np.isfinite(x['dist']).all()
    vx, vy = run_vol(a, fa, b, fb), run_vol(a, fa2, b, fb2)
    assert all(np.array_equal(vx[k], vy[k]) for k in vx)


def test_lattice_counts_match_the_restatement(pairs, batch64, lattice_refs):
    a, fa, b, fb = pairs
    alone = [run_vol(a[k:k + 1], fa, b[k:k + 1], fb) for k in range(len(a))]
    got64 = run_vol(*batch64)
    # the device tells which points it found inside both only as a count: bracket it by the restatement's count without / with the
    # points inside the band (each of them may fall either way)
    for k, ref in enumerate(lattice_refs):
        in_a, in_b = np.abs(ref['w_a']) > 0.5, np.abs(ref['w_b']) > 0.5
        near = (np.abs(np.abs(ref['w_a']) - 0.5) < BAND) | (np.abs(np.abs(ref['w_b']) - 0.5) < BAND)
        sure, maybe = int((in_a & in_b & ~near).sum()), int(near.sum())
        print('pair %d: %d lattice points, %d inside both, %d within %.1e of a threshold; device %d'
              % (k, ref['cells'], ref['n_both'], maybe, BAND, alone[k]['n_both'][0]))
        assert maybe <= 0.01 * ref['cells']
        for got, row in ((alone[k], 0), (got64, ROWS[k])):
            assert got['cells'][row] == ref['cells']
            assert sure <= got['n_both'][row] <= sure + maybe
            if not maybe:
                assert got['n_both'][row] == ref['n_both']
            assert got['volume'][row] == np.float32(got['n_both'][row]) * (np.float32(PITCH) * np.float32(PITCH) * np.float32(PITCH))
            assert abs(got['volume'][row] - got['n_both'][row] * PITCH ** 3) < 1e-6 * ref['volume'] + 1e-12


def test_lattice_counts_of_closed_meshes():
    a, fa = R.cube(0.0325)
    b, fb = R.cube(0.0325, (0.03, 0, 0))
    f32 = lambda v: v.astype(np.float32)[None]  # noqa: E731
    got = run_vol(f32(a), fa, f32(b), fb)
    assert got['cells'][0] == 1183 and got['n_both'][0] == 1183            # exact: no lattice point is near a face
    assert abs(got['volume'][0] - 1183 * PITCH ** 3) < 1e-10
    for name, (sa, sfa, sb, sfb) in closed_cases().items():
        ref = R.intersection(sa[0], sfa, sb[0], sfb, PITCH)
        near = int(((np.abs(np.abs(ref['w_a']) - 0.5) < BAND) | (np.abs(np.abs(ref['w_b']) - 0.5) < BAND)).sum())
        got = run_vol(sa, sfa, sb, sfb)
        print('%s: %d lattice points, %d inside both (device %d), %d near a threshold' % (name, ref['cells'], ref['n_both'], got['n_both'][0], near))
        assert near <= 0.01 * ref['cells'] and got['cells'][0] == ref['cells']
        assert abs(int(got['n_both'][0]) - ref['n_both']) <= near
    far = run_vol(f32(a), fa, f32(b + [1, 0, 0]), fb)                        # disjoint boxes: nothing to examine, volume 0
    assert far['cells'][0] == 0 and far['n_both'][0] == 0 and far['volume'][0] == 0


def test_too_many_cells_gives_nan_and_examines_nothing(pairs, lattice_refs):
    a, fa, b, fb = pairs
    cells = np.array([r['cells'] for r in lattice_refs])
    cap = int(np.sort(cells)[2])                                             # three pairs fit, three do not
    got = run_vol(a, fa, b, fb, max_cells=cap)
    over = cells > cap
    assert over.any() and not over.all()
    assert np.isnan(got['volume'][over]).all() and (got['n_both'][over] == 0).all() and (got['cells'][over] > cap).all()
    full = run_vol(a, fa, b, fb)
    assert np.array_equal(got['n_both'][~over], full['n_both'][~over]) and np.array_equal(got['volume'][~over], full['volume'][~over])
    fine = run_vol(a, fa, b, fb, pitch=0.0002)                               # 5 mm -> 0.2 mm: 15 625 x the points
    assert np.isnan(fine['volume'][cells > 0]).all() and (fine['n_both'] == 0).all() and (cells > 0).sum() >= 4


def test_wrappers_check_their_arguments(pairs):
    from dir_amd import _capi
    a, fa, b, fb = pairs
    A, FA, Bv, FB = dev(a), dev(fa, torch.int32), dev(b), dev(fb, torch.int32)
    with pytest.raises(_capi.DirHipError):
        PN.mesh_penetration(A.cpu(), FA, Bv, FB)
    with pytest.raises(ValueError):
        PN.mesh_penetration(A, FA.long(), Bv, FB)
    with pytest.raises(ValueError):
        PN.mesh_penetration(A[:3], FA, Bv, FB)
    with pytest.raises(_capi.DirHipError):
        PN.intersection_volume(A, FA, Bv, FB, pitch=0.0)
    big = torch.zeros(1, 4097, 3, device='cuda')
    with pytest.raises(_capi.DirHipError):
        PN.mesh_penetration(big, FA, big, FB)


# ------------------------------------------------------------------------------------------------------------------------ wiring
@pytest.fixture(scope='module')
def state():
    with open(os.path.join(HERE, 'golden', 'manifest_dir.json')) as f:
        shapes = {k: tuple(v) for k, v in json.load(f).items()}
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in synth.synth_state_dict(shapes, 1234).items()}


TWELVE = sorted(['left_joint.txt', 'right_joint.txt', 'joint_left_error.txt', 'joint_right_error.txt', 'mesh_left_error.txt',
                 'mesh_right_error.txt', 'joint_2d_left_error.txt', 'joint_2d_right_error.txt', 'mesh_2d_left_error.txt',
                 'mesh_2d_right_error.txt', 'root_loss.txt', 'volume.txt'])


def test_eval_command_line_with_and_without_penetration(tmp_path, state, capsys):
    from dir_amd.apps import dataset as DS
    from dir_amd.apps import eval as EV
    from dir_amd.engine import DirEngine
    from dir_amd.utils.vis_utils import faces_from_layers
    from oracle import image_prep as IP
    n, bs = 10, 4
    write_split(str(tmp_path / 'data'), n, seed=5)
    ck = tmp_path / 'DIR.pth'
    torch.save({'net': state, 'last_epoch': 0}, str(ck))
    args = ['--model', str(ck), '--data_path', str(tmp_path / 'data'), '--bs', str(bs), '--workers', '2', '--dtype', 'bf16']
    plain = EV.main(args + ['--result_dir', str(tmp_path / 'plain')])
    text_plain = capsys.readouterr().out
    m = EV.main(args + ['--result_dir', str(tmp_path / 'pen'), '--penetration', '--penetration_gt'])
    text_pen = capsys.readouterr().out
    # without the flag: the twelve files and the report as they were
    assert sorted(os.listdir(tmp_path / 'plain')) == TWELVE and 'penetration' not in text_plain and not hasattr(plain, 'penetration')
    assert sorted(os.listdir(tmp_path / 'pen')) == sorted(TWELVE + ['penetration.txt', 'penetration_gt.txt'])
    for name in TWELVE:
        assert open(tmp_path / 'plain' / name, 'rb').read() == open(tmp_path / 'pen' / name, 'rb').read(), name
    # the report is the same, and the block comes after the reference's lines, before the rate
    assert m.report() == plain.report() and plain.report() + '\n' in text_plain
    head, tail = text_pen.split(m.report() + '\n')
    assert 'penetration' not in head and 'images/s from files' in text_plain.split(plain.report() + '\n')[1].splitlines()[0]
    block = '\n'.join(tail.splitlines()[:-1])
    assert 'images/s from files' in tail.splitlines()[-1]
    assert block.startswith('penetration:') and 'ground-truth penetration:' in block and 'wrists left open (--seal_wrist auto)' in block
    assert 'intersection volume (5.0 mm lattice)' in block
    # penetration.txt: one row per image, equal to two_hand_penetration on the engine's own outputs (the plain one-batch-at-a-time loop)
    rows = np.loadtxt(str(tmp_path / 'pen' / 'penetration.txt'))
    assert rows.shape == (n, 4)
    eng = DirEngine(state, dtype=torch.bfloat16)
    mano = DS.gt_layers_from_checkpoint(state)
    table = faces_from_layers(mano)
    ds = DS.InterHandSplit(str(tmp_path / 'data'))
    want, want_gt = [], []
    for b0 in range(0, n, bs):
        idx = list(range(b0, min(n, b0 + bs)))
        outs = eng.forward(torch.from_numpy(IP.normalize_u8_bgr(np.stack([ds.frame(i) for i in idx]))).cuda())
        r = PN.two_hand_penetration(outs[2], table, volume_pitch=0.005)
        want.append(np.concatenate([r['count'].cpu().numpy().astype(np.float64), r['depth'].cpu().numpy().astype(np.float64)[:, None] * 1000,
                                    r['volume'].cpu().numpy().astype(np.float64)[:, None] * 1e6], 1))
        gt = DS.gt_batch(mano, torch.from_numpy(np.stack([ds.anno(i) for i in idx])).cuda())
        fl, fr, sealed = PN.hand_faces(table)
        g = PN.mesh_penetration(gt[1], fl, gt[3], fr)
        want_gt.append(g['count'].cpu().numpy())
        assert not sealed
    want = np.concatenate(want)
    as_written = np.array([[float(('%d' if c < 2 else '%.3f') % x) for c, x in enumerate(row)] for row in want])
    assert np.array_equal(rows, as_written, equal_nan=True)
    assert np.array_equal(m.penetration.rows(), want, equal_nan=True)
    assert np.array_equal(np.loadtxt(str(tmp_path / 'pen' / 'penetration_gt.txt'))[:, :2], np.concatenate(want_gt))
    s = m.penetration.summarize()
    assert s['samples'] == n and 0 <= s['rate'] <= 1 and s['depth_max_mm'] >= s['depth_mean_mm'] >= 0
    assert s['vertices_mean'] == want[:, :2].sum(1).mean() and abs(s['depth_mean_mm'] - want[:, 2].mean()) < 1e-9


def test_sealed_wrists_on_a_mesh_that_has_them():
    """hand_faces(seal=...) on a table whose halves are open hemispheres: 'auto' and 'on' seal them, and the kernel on the sealed
    tables matches the restatement on the sealed tables; the synthetic table has no loop: 'auto' leaves it open, 'on' raises"""
    from dir_amd.utils.vis_utils import two_hand_faces
    v, f = R.open_hemisphere(3, 0.03)
    table = np.concatenate([f[:, [1, 0, 2]], f + 778]).astype(np.int32)
    fl, fr, sealed = PN.hand_faces(table, seal='auto')
    assert sealed and fl.shape[0] == fr.shape[0] > len(f) and int(fr.max()) < len(v)
    assert not PN.hand_faces(table, seal='off')[2] and PN.hand_faces(table, seal='on')[2]
    soup = two_hand_faces(np.asarray(synth.synthetic_mano_tables('right')['f']).astype(np.int64))
    assert not PN.hand_faces(soup, seal='auto')[2]
    with pytest.raises(ValueError):
        PN.hand_faces(soup, seal='on')
    a = v.astype(np.float32)[None]
    b = (v * [1, 1, -1] + [0.01, 0.001, 0.0213]).astype(np.float32)[None]          # the mirror dome, pushed into the first
    got = {k: t.cpu().numpy() for k, t in PN.mesh_penetration(dev(a), fl, dev(b), fr, per_vertex=True).items()}
    ref = R.penetration(a[0], fl.cpu().numpy(), b[0], fr.cpu().numpy())
    ew, ed = check_against(ref, got, 0, a.shape[1], 'sealed domes')
    assert ew < WIND_GATE and ed < DIST_GATE and ref['count'].min() > 0


def test_validate_reports_penetration(tmp_path, state):
    from fake_train_split import write_train_split
    from dir_amd.apps import dataset as DS
    from dir_amd.apps import train as T
    from dir_amd.apps.trainset import TrainBatches
    from dir_amd.models.dir import DIR
    d = str(tmp_path / 'split')
    write_train_split(d, 8, seed=11)
    shutil.copytree(os.path.join(d, 'train'), os.path.join(d, 'test'))
    mano = DS.gt_layers_from_checkpoint(state)
    model = DIR(21, 'unused', 0, compute_dtype=torch.float16)
    model.load_state_dict(state, strict=True)
    model.autotune = False
    model = model.cuda()
    vb = lambda: TrainBatches(d, mano, 'test', batch_size=4, workers=2, seed=3, augment=False, shuffle=False)  # noqa: E731
    before = T.validate(model, vb(), quiet=True)
    res = T.validate(model, vb(), quiet=True, penetration=True)
    assert 'penetration_depth_mm' not in before and sorted(set(res) - set(before)) == ['penetration_depth_mm', 'penetration_rate']
    assert all(res[k] == before[k] for k in before)                          # 'error' (which selects best.pth) included
    assert np.isfinite(res['penetration_depth_mm']) and res['penetration_depth_mm'] >= 0 and 0 <= res['penetration_rate'] <= 1
    assert T.build_parser().parse_args(['--init', 'x', '--eval_penetration']).eval_penetration
