"""GPU: dir_amd.apps.predict with antialias -- the flag reaches the crop kernel, the records say which crops it changed, and nothing else moves.

  predict     large frames with hand boxes of 400-600 px (s = 0.27-0.4) and one small frame (s > 1): the crops are
              tests/helpers/crop_area_ref.py::crop_area of the recorded matrices byte for byte, `antialiased` is true exactly where the
              matrix shrinks, the matrices are bit-equal to the run without the flag, whose records have exactly the keys they had
  --track     one sequence of three large frames: the chain of matrices is the restatement's on the read-back stages, as without the flag,
              and every crop is crop_area of its matrix
  command     main(--antialias) writes "antialiased" into the JSON files; without the flag the field is absent"""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'helpers'))
import crop_area_ref as A  # noqa: E402
import crop_ref as R  # noqa: E402

from dir_amd import synth  # noqa: E402
from dir_amd.apps import predict as P  # noqa: E402

pytestmark = pytest.mark.gpu

KEYS = ['image', 'width', 'height', 'box', 'matrix', 'valid', 'tracked', 'left', 'right', 'offset']


@pytest.fixture(scope='module')
def state():
    with open(os.path.join(HERE, 'golden', 'manifest_dir.json')) as fh:
        shapes = {k: tuple(v) for k, v in json.load(fh).items()}
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in synth.synth_state_dict(shapes, 1234).items()}


@pytest.fixture(scope='module')
def eng(state):
    from dir_amd.engine import DirEngine
    return DirEngine(state, dtype=torch.float16)


def large_frames(seed, shapes):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, s + (3,)).astype(np.uint8) for s in shapes]


def test_predict_with_antialias(eng):
    frames = large_frames(46, [(700, 900), (800, 640), (120, 150)])
    boxes = [[150.0, 90.0, 750.5, 600.0], [-40.0, 200.0, 420.0, 700.0], [40.0, 30.0, 100.0, 95.0]]       # the second hangs over the left edge
    plain = P.predict(eng, frames, boxes, keep_crops=True)
    recs = P.predict(eng, frames, boxes, antialias=True, keep_crops=True)
    assert all(sorted(r) == sorted(KEYS + ['crop']) for r in plain)                      # without the flag: exactly the keys there were
    assert all(sorted(r) == sorted(KEYS + ['crop', 'antialiased']) for r in recs)
    assert [r['antialiased'] for r in recs] == [True, True, False]
    for j, (r, q) in enumerate(zip(recs, plain)):
        M = np.float64(r['matrix'])
        want_M, ok = R.matrix_from_box(boxes[j], 0.8, 256)
        assert ok == 1 and np.array_equal(M.view(np.uint64), want_M.view(np.uint64)) and r['matrix'] == q['matrix'], j
        assert r['valid'] and A.is_shrinking(M) == r['antialiased'] and (M[0, 0] < 0.45) == r['antialiased'], j
        assert np.array_equal(r['crop'], A.crop_area(frames[j], M, 256)), j
        assert np.array_equal(r['crop'], q['crop']) == (not r['antialiased']), j          # noise frames: the filter changes every shrunk crop
    # bs = 2: batches of 2 + 1 give the same crops and flags
    recs2 = P.predict(eng, frames, boxes, antialias=True, keep_crops=True, bs=2)
    assert all(np.array_equal(a['crop'], b['crop']) and a['antialiased'] == b['antialiased'] for a, b in zip(recs, recs2))


def test_track_with_antialias(eng):
    seq = large_frames(47, [(700, 900)] * 3)
    first = [[200.0, 100.0, 700.0, 580.0]]
    out = {}
    for flag in (False, True):
        recs = P.predict(eng, [seq], first, track=True, keep_stage=True, keep_crops=True, antialias=flag)[0]
        assert len(recs) == 3 and ('antialiased' in recs[0]) == flag
        M0, ok0 = R.matrix_from_box(first[0], 0.8, 256)
        assert ok0 == 1 and np.array_equal(np.float64(recs[0]['matrix']).view(np.uint64), M0.view(np.uint64))
        assert recs[0]['tracked'] is False and recs[0]['valid'] is True and recs[0]['box'] == first[0]
        for t in range(1, 3):
            prev, cur = recs[t - 1], recs[t]
            st = prev['stage']
            want, ok = R.matrix_from_meshes(st['pd_mesh_xyz_left'], st['pd_mesh_xyz_right'], st['pd_proj_left'], st['pd_proj_right'],
                                            np.float64(prev['matrix']), 0.8, 256)
            assert np.array_equal(np.float64(cur['matrix']).view(np.uint64), want.view(np.uint64)), (flag, t)
            assert cur['tracked'] is bool(ok) and cur['valid'] is True and cur['box'] is None, (flag, t)
        if flag:
            for t, r in enumerate(recs):
                M = np.float64(r['matrix'])
                assert r['antialiased'] == A.is_shrinking(M) and np.array_equal(r['crop'], A.crop_area(seq[t], M, 256)), t
            assert recs[0]['antialiased'] is True
        out[flag] = recs
    assert out[True][0]['matrix'] == out[False][0]['matrix']                             # frame 0 does not depend on any crop
    print('tracked without / with antialias:', [r['tracked'] for r in out[False]], [r['tracked'] for r in out[True]])


def test_command_line_flag(tmp_path, state, eng, capsys):
    from PIL import Image
    frames = large_frames(48, [(400, 520), (90, 100)])
    src = tmp_path / 'in'
    src.mkdir()
    for n, f in zip(('a.png', 'b.png'), frames):
        Image.fromarray(np.ascontiguousarray(f[:, :, ::-1])).save(str(src / n), format='PNG')
    ck = str(tmp_path / 'DIR.pth')
    torch.save({'net': state}, ck)
    with open(tmp_path / 'boxes.json', 'w') as f:
        json.dump({'b': [30.0, 30.0, 70.0, 70.0]}, f)                                    # a.png: the whole frame, s = 0.39; b.png: s = 5.1
    for flag, want in ((['--antialias'], [True, False]), ([], [None, None])):
        out = str(tmp_path / ('out%d' % len(flag)))
        assert P.main(['--model', ck, '--input', str(src), '--out', out, '--boxes', str(tmp_path / 'boxes.json'), '--workers', '2'] + flag) == 2
        assert capsys.readouterr().out.strip().splitlines()[-1].startswith('2 images in ')
        got = []
        for n in ('a', 'b'):
            with open(os.path.join(out, n + '.json')) as f:
                rec = json.load(f)
            assert sorted(rec) == sorted(KEYS + (['antialiased'] if flag else []))
            got.append(rec.get('antialiased'))
        assert got == want
