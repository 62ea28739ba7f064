"""GPU: dir_one_euro_step (csrc/smooth.hip) through dir_amd.utils.smooth against the float64 restatement tests/helpers/one_euro_ref.py.

  parity   B = 3 sequences of T = 12 frames over the segments [(300, 3, 1000), (5, 2, 1), (3, 1, 1), (1, 3, 1000)] (300 points: more than
           one pass of the 256 lanes; three component counts), smooth random walks plus noise, metres around +-0.1 and pixels around
           0..2000.  Row 0 is invalid at two frames (bridged: dt = 3 / fps), row 1 has a single NaN at one frame, row 2 is invalid for
           four frames with max_gap = 3 (it starts again).  Every frame's y and `updated`, and the final jitter sums and counts.  Then
           the PredictionSmoother layout (9 segments, F = 4887, odd) once, B = 2, T = 4.
  bits     a constant input is returned bit for bit; the first frame is y = x; a row alone equals the same row in slot 3 of a batch of 5,
           state included; a batch that shrinks from the tail leaves the other rows' bits alone; y may be x.

The gate.  err = max |kernel - restatement| / max |x| of the segment.  The kernel works in float32 (a few ulp per step, carried through a
recursion whose smallest gain in this test is alpha = 0.17 at 30 fps and 1 Hz): the cap is 1e-5; a kernel beyond it is wrong.  Below the
cap the gate is 4 x the largest error measured on the MI355X, the margin tests/test_gpu_alignment.py uses for float32 against float64.
Measured (MI355X): 6.92e-8, 7.64e-8, 5.59e-8, 3.32e-8 for the four segments of the parity case; 7.77e-8 at most over the nine streams of the
PredictionSmoother layout; 8.92e-8 at most over the streams of tests/test_gpu_predict_smooth.py (camera_px_left), 8.24e-8 after its lost frame,
7.51e-8 for the box filter.  The largest, 8.92e-8, gives the gate 3.57e-7.
`updated`, passed-through rows (bit for bit, NaN included) and the jitter counts are exact.  The jitter sums are second differences of
values within `gate` of the restatement's, weights 1, 2, 1: they are held to 4 x gate x max |x| per point and counted frame; the raw sums
are sums in double of float32 inputs and are held to 1e-12 relative."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'helpers'))
from one_euro_ref import OneEuroRef  # noqa: E402

from dir_amd.utils import smooth as SM  # noqa: E402

pytestmark = pytest.mark.gpu

SEGS = [(300, 3, 1000.0), (5, 2, 1.0), (3, 1, 1.0), (1, 3, 1000.0)]
B, T, MAX_GAP = 3, 12, 3
CAP = 1e-5
MEASURED = 8.92e-8                                           # the largest err measured on the MI355X (see the docstring)
GATE = min(4 * MEASURED, CAP)


def walks(segs, rows, frames, seed):
    """smooth random walks plus noise, float32 [frames, rows, F]: metres (speed scale 1000) around +-0.1, pixels around 0..2000"""
    rng = np.random.default_rng(seed)
    parts = []
    for n, d, scale in segs:
        if scale == 1000.0:
            start, step, noise = rng.uniform(-0.1, 0.1, (1, rows, n * d)), 0.003, 0.001
        else:
            start, step, noise = rng.uniform(0, 2000, (1, rows, n * d)), 3.0, 1.0
        vel = np.cumsum(rng.normal(size=(frames, rows, n * d)) * step * 0.3, 0)
        parts.append(start + np.cumsum(vel, 0) + rng.normal(size=(frames, rows, n * d)) * noise)
    return np.concatenate(parts, 2).astype(np.float32)


def seg_errors(segs, got, want, xs):
    """-> per segment max |got - want| / max |x| over [..., F] arrays (non-finite positions must agree and are left out)"""
    out, at = [], 0
    for n, d, _ in segs:
        sl = slice(at, at + n * d)
        g, w = np.asarray(got, np.float64)[..., sl], np.asarray(want, np.float64)[..., sl]
        fin = np.isfinite(w)
        assert np.array_equal(fin, np.isfinite(g))
        out.append(float(np.abs(g - w)[fin].max() / np.abs(xs[..., sl][np.isfinite(xs[..., sl])]).max()))
        at += n * d
    return out


def check_jitter(f, ref, segs, xs, rows):
    j = f.jitter()
    assert j['frames'][:rows].tolist() == ref.count[:rows].tolist()
    at = 0
    for s, (n, d, _) in enumerate(segs):
        top = np.abs(xs[..., at:at + n * d][np.isfinite(xs[..., at:at + n * d])]).max()
        for b in range(rows):
            raw, fil = j['sums'][b, s]
            print('jitter row %d segment %d: raw %.9g (ref %.9g)  filtered %.9g (ref %.9g)' % (b, s, raw, ref.jitter[b, s, 0], fil, ref.jitter[b, s, 1]))
            assert abs(raw - ref.jitter[b, s, 0]) <= 1e-12 * max(ref.jitter[b, s, 0], top)
            assert abs(fil - ref.jitter[b, s, 1]) <= 4 * GATE * top * n * max(int(ref.count[b]), 1)
        at += n * d


def test_parity_with_the_restatement():
    xs = walks(SEGS, B, T, 11)
    valid = np.ones((T, B), np.int32)
    valid[4:6, 0] = 0                                                     # bridged: age 3 <= max_gap
    xs[6, 1, 917 % xs.shape[2]] = np.nan                                  # one NaN: the whole row passes through
    valid[3:7, 2] = 0                                                     # age 5 > max_gap: starts again at frame 7
    f = SM.OneEuro(SEGS, B, max_gap=MAX_GAP)
    ref = OneEuroRef(SEGS, B, max_gap=MAX_GAP)
    assert f.F == ref.F == xs.shape[2]
    worst = [0.0] * len(SEGS)
    ups = []
    for t in range(T):
        x = torch.from_numpy(xs[t]).cuda()
        y, upd = f.step(x, torch.from_numpy(valid[t]).cuda())
        want, wupd = ref.step(xs[t], valid[t])
        y, upd = y.cpu().numpy(), upd.cpu().numpy()
        assert upd.tolist() == wupd.tolist(), t
        ups.append(upd.tolist())
        for b in range(B):
            if upd[b] != 1:                                               # passed through or initialised: y = x bit for bit
                assert np.array_equal(y[b].view(np.uint32), xs[t, b].view(np.uint32)), (t, b)
        worst = [max(a, e) for a, e in zip(worst, seg_errors(SEGS, y, want, xs))]
    print('updated per frame:', ups)
    print('largest |kernel - restatement| / max |x| per segment:', ['%.3g' % e for e in worst], 'gate %.3g' % GATE)
    assert [u[0] for u in ups] == [2, 1, 1, 1, 0, 0, 1, 1, 1, 1, 1, 1] and [u[1] for u in ups] == [2] + [1] * 5 + [0] + [1] * 5
    assert [u[2] for u in ups] == [2, 1, 1, 0, 0, 0, 0, 2, 1, 1, 1, 1]
    assert max(worst) <= GATE, worst
    check_jitter(f, ref, SEGS, xs, B)
    assert f.field('age').cpu().numpy().reshape(-1).tolist() == ref.age.tolist() and f.field('run').cpu().numpy().reshape(-1).tolist() == ref.run.tolist()


def fake_stage(rng, rows):
    st = {'pd_offset': rng.normal(size=(rows, 3)) * 0.05}
    for s in ('left', 'right'):
        st['pd_mesh_xyz_' + s] = rng.uniform(-0.1, 0.1, (rows, 778, 3))
        st['pd_joint_xyz_' + s] = rng.uniform(-0.1, 0.1, (rows, 21, 3))
        st['pd_joint_uv_' + s] = rng.uniform(-0.8, 0.8, (rows, 21, 2))
        st['pd_proj_' + s] = np.concatenate([rng.uniform(4, 8, (rows, 1)), rng.uniform(-0.3, 0.3, (rows, 2))], 1)
    return {k: torch.from_numpy(v.astype(np.float32)).cuda() for k, v in st.items()}


def test_prediction_smoother_layout():
    rng = np.random.default_rng(5)
    rows, frames = 2, 4
    segs = [(p, d, v) for _, p, d, v in SM.STREAMS]
    sm = SM.PredictionSmoother(rows, 256)
    ref = OneEuroRef(segs, rows)
    base = fake_stage(rng, rows)
    xs, got, want = [], [], []
    for t in range(frames):
        stage = {k: v + torch.from_numpy((rng.normal(size=tuple(v.shape)) * 0.002).astype(np.float32)).cuda() for k, v in base.items()}
        s = rng.uniform(0.4, 1.5, rows)
        M = torch.from_numpy(np.stack([s, 0 * s, rng.uniform(-300, 0, rows), 0 * s, s, rng.uniform(-300, 0, rows)], 1)).cuda()
        x = sm.pack(stage, M).cpu().numpy()
        fr = sm.step(stage, M)
        y = torch.cat([fr[n].flatten(1) for n, _, _, _ in SM.STREAMS], 1).cpu().numpy()
        w, wupd = ref.step(x)
        assert fr['updated'].cpu().tolist() == wupd.tolist() == [2 if t == 0 else 1] * rows
        assert tuple(fr['mesh_xyz_left'].shape) == (rows, 778, 3) and tuple(fr['joints_px_right'].shape) == (rows, 21, 2)
        assert tuple(fr['camera_px_left'].shape) == (rows, 3) and tuple(fr['offset'].shape) == (rows, 3)
        assert np.array_equal(torch.cat([fr['raw'][n].flatten(1) for n, _, _, _ in SM.STREAMS], 1).cpu().numpy(), x)
        cs = sm.crop_stage()
        assert sorted(cs) == sorted(base)
        if t == 0:                                                        # initialised: the stage itself, bit for bit
            assert all(torch.equal(cs[k], stage[k]) for k in cs)
        else:                                                             # mapped back into the crop: the smoothed pixels again, to float32 rounding
            from dir_amd.utils import crop as CR
            back = CR.to_frame_pixels(cs['pd_joint_uv_left'], M, 256)
            assert float((back - fr['joints_px_left']).abs().max()) <= 2e-7 * 2000 + 1e-4
            sc, tr = CR.frame_camera(cs['pd_proj_right'], M, 256)
            assert float((sc - fr['camera_px_right'][:, 0]).abs().max()) <= 4e-7 * float(sc.abs().max())
            assert float((tr - fr['camera_px_right'][:, 1:3]).abs().max()) <= 1e-3
            assert torch.equal(cs['pd_mesh_xyz_right'], fr['mesh_xyz_right']) and cs['pd_mesh_xyz_right'].is_contiguous()
        xs.append(x), got.append(y), want.append(w)
    xs = np.stack(xs)
    worst = seg_errors(segs, np.stack(got), np.stack(want), xs)
    print('PredictionSmoother layout, largest err per stream:', dict(zip([n for n, _, _, _ in SM.STREAMS], ['%.3g' % e for e in worst])))
    assert max(worst) <= GATE, worst
    check_jitter(sm.filter, ref, segs, xs, rows)
    assert sm.jitter()['streams'][0] == 'mesh_xyz_left' and sm.jitter()['frames'].tolist() == [2, 2]


def bits(t):
    return t.contiguous().view(torch.uint8).cpu().numpy()


def test_constant_input_and_first_frame_bits():
    x = torch.from_numpy(walks(SEGS, 2, 1, 3)[0]).cuda()
    f = SM.OneEuro(SEGS, 2)
    for t in range(5):
        y, upd = f.step(x)
        assert np.array_equal(bits(y), bits(x)) and upd.cpu().tolist() == [2 if t == 0 else 1] * 2, t
    j = f.jitter()
    assert j['frames'].tolist() == [3, 3] and not j['sums'].any()


def test_a_row_gives_the_same_bits_in_any_slot_of_any_batch():
    xs = walks(SEGS, 5, 6, 7)
    alone, five = SM.OneEuro(SEGS, 1), SM.OneEuro(SEGS, 5)
    valid = np.ones((6, 5), np.int32)
    valid[3, 3] = 0                                                       # the pass-through path too
    for t in range(6):
        ya, ua = alone.step(torch.from_numpy(xs[t, 3:4]).cuda(), torch.from_numpy(valid[t, 3:4]).cuda())
        yf, uf = five.step(torch.from_numpy(xs[t]).cuda(), torch.from_numpy(valid[t]).cuda())
        assert np.array_equal(bits(ya[0]), bits(yf[3])) and ua.cpu().tolist() == uf[3:4].cpu().tolist(), t
    assert np.array_equal(bits(alone.state[0]), bits(five.state[3]))
    assert alone.jitter()['frames'].tolist() == [1]                         # frame 2; the run starts again after frame 3


def test_a_batch_that_shrinks_from_the_tail():
    xs = walks(SEGS, 3, 8, 9)
    three, two = SM.OneEuro(SEGS, 3), SM.OneEuro(SEGS, 2)
    for t in range(8):
        rows = 3 if t < 4 else 2
        y3, u3 = three.step(torch.from_numpy(xs[t, :rows]).cuda())
        y2, u2 = two.step(torch.from_numpy(xs[t, :2]).cuda())
        assert np.array_equal(bits(y3[:2]), bits(y2)) and u3[:2].cpu().tolist() == u2.cpu().tolist(), t
    assert np.array_equal(bits(three.state[:2]), bits(two.state))
    assert three.field('age').cpu().numpy().reshape(-1).tolist() == [1, 1, 1] and three.jitter()['frames'].tolist() == [6, 6, 2]
    with pytest.raises(ValueError):
        two.step(torch.from_numpy(xs[0]).cuda())                          # sequences may end, not begin


def test_y_may_alias_x():
    xs = walks(SEGS, 2, 5, 13)
    xs[3, 1, 5] = np.inf
    apart, place = SM.OneEuro(SEGS, 2), SM.OneEuro(SEGS, 2)
    for t in range(5):
        x = torch.from_numpy(xs[t]).cuda()
        y, u = apart.step(x)
        buf = x.clone()
        y2, u2 = place.step(buf, out=buf)
        assert y2 is buf and np.array_equal(bits(y), bits(buf)) and u.cpu().tolist() == u2.cpu().tolist(), t
        assert np.array_equal(bits(x), xs[t].view(np.uint8).reshape(2, -1))          # separate buffers: x untouched
    assert np.array_equal(bits(apart.state), bits(place.state))
