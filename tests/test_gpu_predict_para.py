"""GPU: dir_amd.apps.predict --track --smooth --smooth_space para, with synthetic weights and generated frames (set up as
tests/test_gpu_predict_smooth.py): 2 sequences x 6 frames at batch 2.

  records      predict(track=True, smooth={'space': 'para'}): the new fields ("mano", "shape_frozen"), `raw` equal to the unflagged run bit for bit,
               the regenerated left / right consistent with one another (2-D joints = camera_px applied to the 3-D joints), and the 15 rigid bone
               lengths of left / right constant after the freeze -- within the float32 distance of two regenerated joints, para_smooth_ref's joints gate
               -- while those of `raw` keep changing
  unchanged    smooth=True gives the records and the jitter fields it gave (tests/test_gpu_predict_smooth.py pins their values; here: no new key
               appears and {'space': 'point'} is smooth=True bit for bit)
  command      --smooth_space para / --shape_frames without --track --smooth exit with an error; main() with the flag writes the fields, jitter.json
               with the bone flicker, and prints it"""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'helpers'))
import para_smooth_ref as R  # noqa: E402
from fake_split import write_split  # noqa: E402

from dir_amd import synth  # noqa: E402
from dir_amd.apps import dataset as DS  # noqa: E402
from dir_amd.apps import predict as P  # noqa: E402

pytestmark = pytest.mark.gpu

CANVASES = [((300, 400), (70, 40)), ((512, 334), (0, 256))]              # (H, W), (ox, oy)
T, SHAPE_FRAMES = 6, 2
SIDES = ('left', 'right')
# a rigid bone's length from two regenerated float32 joints, each within gate('joints') of the exact one per component; between two frames twice that
LENGTH_GATE = 4.0 * math.sqrt(3.0) * R.gate('joints')


@pytest.fixture(scope='module')
def state():
    with open(os.path.join(HERE, 'golden', 'manifest_dir.json')) as fh:
        shapes = {k: tuple(v) for k, v in json.load(fh).items()}
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in synth.synth_state_dict(shapes, 1234).items()}


@pytest.fixture(scope='module')
def eng(state):
    from dir_amd.engine import DirEngine
    return DirEngine(state, dtype=torch.float16)


@pytest.fixture(scope='module')
def video(tmp_path_factory):
    root = str(tmp_path_factory.mktemp('tiles'))
    write_split(root, 4, seed=5)
    ds = DS.InterHandSplit(root)
    tiles = [np.ascontiguousarray(ds.frame(i)) for i in range(4)]
    rng = np.random.default_rng(11)
    seqs, first = [], []
    for q, ((h, w), (ox, oy)) in enumerate(CANVASES):
        frames = []
        for t in range(T):
            c = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
            c[oy:oy + 256, ox:ox + 256] = tiles[(q + t) % 4]
            frames.append(c)
        seqs.append(frames)
        first.append([ox + 20.0, oy + 20.0, ox + 236.0, oy + 236.0] if q == 0 else [ox + 125.0, oy + 125.0, ox + 131.0, oy + 131.0])
    return seqs, first


@pytest.fixture(scope='module')
def plain(eng, video):
    return P.predict(eng, video[0], video[1], ratio=0.8, stage=2, bs=2, track=True)


def rigid_lengths(rec_side):
    return R.bone_lengths(torch.tensor(rec_side['joints_xyz'], dtype=torch.float64), R.RIGID).numpy()


def test_para_records(eng, video, plain):
    seqs, first = video
    recs, jit = P.predict(eng, seqs, first, ratio=0.8, stage=2, bs=2, track=True, smooth={'space': 'para', 'shape_frames': SHAPE_FRAMES}, return_jitter=True)
    for q in range(2):
        for t in range(T):
            a, b = plain[q][t], recs[q][t]
            assert b['smoothed'] is True and b['raw'] == {k: a[k] for k in ('left', 'right', 'offset')}, (q, t)
            assert all(a[k] == b[k] for k in ('image', 'width', 'height', 'box', 'matrix', 'valid', 'tracked'))
            assert b['shape_frozen'] == [t + 1 >= SHAPE_FRAMES] * 2
            for s in SIDES:
                m = b['mano'][s]
                assert [len(m[k]) for k in ('root_6d', 'pose_aa', 'betas', 'camera_px')] == [6, 45, 10, 3]
                assert m['camera_px'] == [b[s]['camera_px']['scale']] + b[s]['camera_px']['trans']
                # the regenerated outputs agree with one another: 2-D joints are the camera applied to the 3-D joints (one float32 product and sum)
                j3, j2 = np.array(b[s]['joints_xyz'], np.float64), np.array(b[s]['joints_px'], np.float64)
                want = m['camera_px'][0] * j3[:, :2] + np.array(m['camera_px'][1:])
                assert np.abs(j2 - want).max() <= 4 * 2.0 ** -24 * np.abs(want).max(), (q, t, s)
                if t == 0:
                    assert b[s]['joints_xyz'] == a[s]['joints_xyz']           # initialised: the forward at the network's own parameters
        for s in SIDES:
            frozen = [recs[q][t]['mano'][s]['betas'] for t in range(SHAPE_FRAMES - 1, T)]
            assert all(f == frozen[0] for f in frozen)
            L = np.stack([rigid_lengths(recs[q][t][s]) for t in range(SHAPE_FRAMES - 1, T)])
            Lraw = np.stack([rigid_lengths(recs[q][t]['raw'][s]) for t in range(SHAPE_FRAMES - 1, T)])
            spread, spread_raw = float((L.max(0) - L.min(0)).max()), float((Lraw.max(0) - Lraw.min(0)).max())
            print('sequence %d %s: rigid bone length spread after the freeze %.3g m (raw %.3g m), gate %.3g' % (q, s, spread, spread_raw, LENGTH_GATE))
            assert spread <= LENGTH_GATE and spread < spread_raw
        f = jit[q]['bone_flicker']
        assert jit[q]['space'] == 'para' and f['hands'] == list(SIDES) and f['frames'] == [T - 2] * 2 and jit[q]['frames'] == T - 2
        assert all(v is not None and v >= 0 for v in f['raw_mm'] + f['filtered_mm'])
    raw, fil = P.flicker_summary(jit)
    print('bone flicker, raw -> smoothed: %.4g -> %.4g mm/frame per bone' % (raw, fil))
    assert np.isfinite([raw, fil]).all()


def test_without_the_flag_nothing_new_appears(eng, video, plain):
    seqs, first = video
    recs, jit = P.predict(eng, seqs, first, ratio=0.8, stage=2, bs=2, track=True, smooth=True, return_jitter=True)
    point, jit_p = P.predict(eng, seqs, first, ratio=0.8, stage=2, bs=2, track=True, smooth={'space': 'point'}, return_jitter=True)
    assert recs == point and jit == jit_p
    for q in range(2):
        assert set(jit[q]) == {'streams', 'points', 'frames', 'raw', 'filtered', 'sums'}
        for t in range(T):
            assert set(recs[q][t]) == set(plain[q][t]) | {'raw', 'smoothed'}
            assert recs[q][t]['raw'] == {k: plain[q][t][k] for k in ('left', 'right', 'offset')}
    with pytest.raises(ValueError, match='shape_frames'):
        P.Tracker(eng, smooth={'shape_frames': 3})
    with pytest.raises(ValueError, match='space'):
        P.Tracker(eng, smooth={'space': 'mesh'})
    with pytest.raises(ValueError, match='track'):
        P.predict(eng, [seqs[0][0]], smooth={'space': 'para'})


def test_command_line(state, video, tmp_path, capsys):
    base = ['--model', 'none.pth', '--input', str(tmp_path), '--out', str(tmp_path / 'o')]
    for extra in (['--smooth_space', 'para'], ['--track', '--smooth_space', 'para'], ['--smooth', '--smooth_space', 'para'], ['--track', '--shape_frames', '3'],
                  ['--track', '--smooth', '--shape_frames', '3'], ['--track', '--smooth', '--smooth_space', 'para', '--shape_frames', '-1']):
        with pytest.raises(SystemExit):
            P.main(base + extra)
    capsys.readouterr()
    from PIL import Image
    ck = str(tmp_path / 'ck.pth')
    torch.save({'net': state}, ck)
    src = tmp_path / 'seq'
    src.mkdir()
    for t, f in enumerate(video[0][0]):
        Image.fromarray(np.ascontiguousarray(f[:, :, ::-1])).save(str(src / ('%03d.png' % t)), format='PNG')
    out = tmp_path / 'out'
    n = P.main(['--model', ck, '--input', str(src), '--out', str(out), '--track', '--smooth', '--smooth_space', 'para', '--shape_frames', '2', '--bs', '2',
                '--pictures', '--joints', '--obj', '--workers', '2'])
    printed = capsys.readouterr().out
    assert n == T and 'bone flicker, raw -> smoothed:' in printed and 'jitter, raw -> smoothed:' in printed
    assert all(os.path.getsize(str(out / ('003' + e))) > 0 for e in ('.png', '.obj'))      # drawn from ParameterSmoother.crop_stage
    r = json.load(open(str(out / '003.json')))
    assert r['smoothed'] is True and r['shape_frozen'] == [True, True] and set(r['mano']) == set(SIDES) and set(r['raw']) == {'left', 'right', 'offset'}
    j = json.load(open(str(out / 'jitter.json')))
    assert j['space'] == 'para' and j['bone_flicker']['frames'] == [T - 2] * 2 and len(j['bone_flicker']['raw_mm']) == 2
