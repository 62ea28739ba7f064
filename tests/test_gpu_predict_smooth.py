"""GPU: dir_amd.apps.predict --track with --smooth / --smooth_box, with synthetic weights (set up as tests/test_gpu_predict.py).

  records      predict(track=True, smooth=True): `raw` equals the unflagged run's fields exactly (the crops and forwards are the same), frame
               0's smoothed values equal its raw ones, and the smoothed fields equal the restatement (tests/helpers/one_euro_ref.py)
               applied on the host to the raw frame-space streams, within tests/test_gpu_smooth.py's gate
  a lost frame a sequence whose frame 2 is made invalid keeps its nulls there and resumes at frame 3 with dt = 2 / fps
  drawing      overlay_predictions of crop_stage equals the raw overlay exactly at frame 0 and runs (and differs) later
  command      main() --track --smooth --pictures --obj: the JSON fields, jitter.json, the printed lines; --smooth without --track exits
  --smooth_box smooth_matrices alone against the restatement; in predict() frames 0 and 1 keep the unsmoothed run's matrices bit for bit,
               every matrix stays axis-aligned and valid, a held box leaves the box filter's values alone

Nothing downstream of a smoothed crop is compared with a host chain: a last-bit difference of a matrix can flip crop bytes.

smooth_matrices' tolerance.  The filter's output is float32 and lies within the gate of the float64 restatement, so the matrix cannot equal a
float64 chain to 1e-9; what is held to 1e-9 relative is the float64 part: the matrix against cut_img's formula applied in numpy to the
filter's own float32 output.  The filter's output itself is held to the gate."""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'helpers'))
from fake_split import write_split  # noqa: E402
from one_euro_ref import OneEuroRef  # noqa: E402
from test_gpu_smooth import GATE  # noqa: E402

from dir_amd import synth  # noqa: E402
from dir_amd.apps import dataset as DS  # noqa: E402
from dir_amd.apps import predict as P  # noqa: E402
from dir_amd.utils import crop as CR  # noqa: E402
from dir_amd.utils import smooth as SM  # noqa: E402
from dir_amd.utils import vis_utils as V  # noqa: E402

pytestmark = pytest.mark.gpu

CANVASES = [((300, 400), (70, 40)), ((512, 334), (0, 256))]              # (H, W), (ox, oy)
T = 4
SEGS = [(p, d, v) for _, p, d, v in SM.STREAMS]


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
    """two sequences of four small canvases; sequence 0 starts from a hands-sized box, sequence 1 from a 6 px box (its tracked boxes hold:
    tests/test_gpu_predict.py::test_track)"""
    root = str(tmp_path_factory.mktemp('tiles'))
    write_split(root, 4, seed=5)
    ds = DS.InterHandSplit(root)
    tiles = [np.ascontiguousarray(ds.frame(i)) for i in range(4)]
    rng = np.random.default_rng(9)
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
    """the unflagged run, made once"""
    return P.predict(eng, video[0], video[1], ratio=0.8, stage=2, track=True, keep_stage=True, keep_crops=True)


def row_of(rec_fields, mesh):
    """the frame-space streams of one record in PredictionSmoother's order, float32 [F] (None -> NaN)"""
    parts = []
    for s in ('left', 'right'):
        h = rec_fields[s]
        parts += [mesh['pd_mesh_xyz_' + s].reshape(-1), np.array(h['joints_xyz'], np.float64).reshape(-1), np.array(h['joints_px'], np.float64).reshape(-1),
                  np.array([h['camera_px']['scale']] + h['camera_px']['trans'], np.float64)]
    parts.append(np.array(rec_fields['offset'], np.float64))
    return np.concatenate([np.asarray(p, np.float64) for p in parts]).astype(np.float32)


def stream_errors(got, want, xs):
    out, at = {}, 0
    for name, p, d, _ in SM.STREAMS:
        sl = slice(at, at + p * d)
        out[name] = float(np.abs(got[..., sl].astype(np.float64) - want[..., sl]).max() / np.abs(xs[..., sl]).max())
        at += p * d
    return out


def test_smoothed_records(eng, video, plain):
    seqs, first = video
    recs, jit = P.predict(eng, seqs, first, ratio=0.8, stage=2, track=True, keep_stage=True, keep_crops=True, smooth=True, return_jitter=True)
    worst = {}
    for q in range(2):
        ref = OneEuroRef(SEGS, 1)
        for t in range(T):
            a, b = plain[q][t], recs[q][t]
            assert 'raw' not in a and 'smoothed' not in a and b['smoothed'] is True
            assert b['raw'] == {k: a[k] for k in ('left', 'right', 'offset')}, (q, t)
            assert all(a[k] == b[k] for k in ('image', 'width', 'height', 'box', 'matrix', 'valid', 'tracked')) and np.array_equal(a['crop'], b['crop'])
            assert all(np.array_equal(a['stage'][k], b['stage'][k]) for k in a['stage'])
            if t == 0:
                assert all(b[k] == b['raw'][k] for k in ('left', 'right', 'offset'))
                assert all(np.array_equal(b['stage_smoothed'][k], b['stage'][k]) for k in b['stage'])
            x = row_of(b['raw'], b['stage'])
            assert np.isfinite(x).all()
            want, upd = ref.step(x[None])
            assert upd[0] == (2 if t == 0 else 1)
            got = row_of(b, b['stage_smoothed'])
            for k, e in stream_errors(got, want[0], x).items():
                worst[k] = max(worst.get(k, 0.0), e)
        assert jit[q]['frames'] == T - 2 and jit[q]['streams'][0] == 'mesh_xyz_left' and len(jit[q]['raw']) == len(SEGS)
        for s, (p, (raw, fil)) in enumerate(zip(jit[q]['points'], jit[q]['sums'])):
            assert abs(raw - ref.jitter[0, s, 0]) <= 1e-9 * max(raw, 1.0) and jit[q]['raw'][s] == raw / p / (T - 2)
    print('predict --smooth, largest |smoothed - restatement| / max |x| per stream:', {k: '%.3g' % e for k, e in worst.items()}, 'gate %.3g' % GATE)
    assert max(worst.values()) <= GATE, worst


def test_a_lost_frame_keeps_its_nulls_and_is_bridged(eng, video):
    seqs, first = video
    tr = P.Tracker(eng, ratio=0.8, stage=2, smooth={'beta': 0.0})        # beta 0: the gain below is alpha(min_cutoff) whatever the speed
    ref = OneEuroRef(SEGS, 2, beta=0.0)
    for t in range(T):
        if t == 2:                                                        # no crop can be made for either sequence: a zero matrix, valid 0
            saved = tr._next
            tr._next = (torch.zeros_like(saved[0]), torch.zeros_like(saved[1]), torch.zeros_like(saved[2]))
        if t == 3:                                                        # the boxes frame 1 asked for are found again
            tr._next = saved
        batch = CR.FrameBatch([s[t] for s in seqs])
        crops, outs = tr.step(batch, first if t == 0 else None)
        recs = P._records(['0', '1'], batch, first if t == 0 else None, tr, outs, 2, True)
        upd = tr.smoothed['updated'].cpu().tolist()
        if t == 2:
            assert upd == [0, 0] and tr.valid.cpu().tolist() == [0, 0]
            for r in recs:
                assert r['valid'] is False and r['left']['joints_px'] == [[None, None]] * 21 and r['left']['camera_px']['scale'] is None
                assert r['raw'] == {k: r[k] for k in ('left', 'right', 'offset')}          # passed through: nulls stay nulls, the rest is raw
            ref.step(np.zeros((2, ref.F)), [0, 0])
            continue
        assert upd == [2, 2] if t == 0 else upd == [1, 1]
        x = np.stack([row_of(r['raw'], r['stage']) for r in recs])
        want, wupd = ref.step(x)
        assert wupd.tolist() == upd
        if t == 3:                                                        # dt = 2 / fps: the restatement bridged one frame
            err = max(max(stream_errors(row_of(r, r['stage_smoothed']), want[j], x[j]).values()) for j, r in enumerate(recs))
            print('after a lost frame: largest err %.3g, gate %.3g' % (err, GATE))
            assert err <= GATE
            # and the gain itself, on the offset stream: alpha at dt = 2 / fps (0.295), not at 1 / fps (0.173)
            y1, xo, yo = ref.y2[0, -3:], x[0, -3:].astype(np.float64), np.array(recs[0]['offset'])
            k = int(np.abs(xo - y1).argmax())
            gain = (yo[k] - y1[k]) / (xo[k] - y1[k])
            print('gain after the lost frame %.6f (alpha(2 / fps) = %.6f)' % (gain, 1 / (1 + 15 / (2 * np.pi))))
            assert abs(gain - 1 / (1 + 15 / (2 * np.pi))) < 1e-3
    assert tr.smoother.jitter()['frames'].tolist() == [0, 0]             # no three consecutive updates


def test_crop_stage_is_drawn(eng, state, video):
    seqs, first = video
    mano = DS.gt_layers_from_checkpoint(state)
    r = V.mano_two_hands_shaded_renderer(right_faces=mano['right'].get_faces(), dense_color=np.zeros((778, 3)), img_size=256, device='cuda')
    tr = P.Tracker(eng, ratio=0.8, stage=2, smooth=True)
    for t in range(3):
        crops, outs = tr.step(CR.FrameBatch([s[t] for s in seqs]), first if t == 0 else None)
        shown = tr.drawn(outs)
        raw_over = V.overlay_predictions(outs[2], crops, r)
        over = V.overlay_predictions(shown, crops, r)
        drawn = V.draw_joints(over.clone(), shown['pd_joint_uv_left'], shown['pd_joint_uv_right'])
        _, _, vl, vr = V.prediction_camera(shown)
        assert over.dtype == torch.uint8 and tuple(over.shape) == (2, 256, 256, 3) and tuple(vl.shape) == tuple(vr.shape) == (2, 778, 3)
        assert tuple(drawn.shape) == (2, 256, 256, 3)
        moved = [not torch.equal(shown[k].float(), outs[2][k].float()) for k in ('pd_mesh_xyz_left', 'pd_mesh_xyz_right', 'pd_proj_left', 'pd_proj_right')]
        if t == 0:
            assert not any(moved) and torch.equal(over, raw_over)
        else:
            assert all(moved)
            if not torch.equal(over, raw_over):                           # the pictures differ only because smoothing moved something
                assert any(moved)
    assert P.Tracker(eng, ratio=0.8, stage=2).drawn(outs) is outs[2]
    with pytest.raises(ValueError):
        P.Tracker(eng, track=False, smooth=True)


def save_png(path, bgr):
    from PIL import Image
    Image.fromarray(np.ascontiguousarray(bgr[:, :, ::-1])).save(path, format='PNG')


def test_smooth_command(tmp_path, state, eng, video, capsys):
    from PIL import Image
    seqs, first = video
    src = tmp_path / 'video'
    for q, name in enumerate(('a', 'b')):
        (src / name).mkdir(parents=True)
        for t in range(T):
            save_png(str(src / name / ('%d.png' % t)), seqs[q][t])
    with open(tmp_path / 'boxes.json', 'w') as f:
        json.dump({'a/0.png': first[0], 'b/0': first[1]}, f)
    ck = str(tmp_path / 'DIR.pth')
    torch.save({'net': state}, ck)
    common = ['--model', ck, '--input', str(src), '--boxes', str(tmp_path / 'boxes.json'), '--track', '--pictures', '--obj', '--workers', '2']
    out0, out1 = str(tmp_path / 'plain'), str(tmp_path / 'smooth')
    assert P.main(common + ['--out', out0]) == 2 * T
    capsys.readouterr()
    assert P.main(common + ['--out', out1, '--smooth']) == 2 * T                       # the flag alone: the defaults
    lines = capsys.readouterr().out.strip().splitlines()
    assert lines[-1].startswith('%d images in ' % (2 * T)) and lines[-1].endswith('images/s')
    assert lines[-2].startswith('jitter, raw -> smoothed: ') and 'mm/frame^2' in lines[-2] and 'px/frame^2' in lines[-2] and 'nan' not in lines[-2]
    want = P.predict(eng, seqs, first, ratio=0.8, stage=2, track=True, smooth=True)
    plain_keys = ['image', 'width', 'height', 'box', 'matrix', 'valid', 'tracked', 'left', 'right', 'offset']
    for q, name in enumerate(('a', 'b')):
        assert sorted(os.listdir(os.path.join(out1, name))) == sorted(['%d%s' % (t, e) for t in range(T) for e in ('.json', '.png', '.obj')] + ['jitter.json'])
        assert 'jitter.json' not in os.listdir(os.path.join(out0, name))
        with open(os.path.join(out1, name, 'jitter.json')) as f:
            j = json.load(f)
        assert sorted(j) == ['filtered', 'frames', 'points', 'raw', 'streams', 'sums'] and j['frames'] == T - 2 and j['streams'] == [n for n, _, _, _ in SM.STREAMS]
        assert all(v is not None and v >= 0 for v in j['raw'] + j['filtered'])
        for t in range(T):
            with open(os.path.join(out0, name, '%d.json' % t)) as f:
                r0 = json.load(f)
            with open(os.path.join(out1, name, '%d.json' % t)) as f:
                r1 = json.load(f)
            assert sorted(r0) == sorted(plain_keys) and sorted(r1) == sorted(plain_keys + ['smoothed', 'raw'])
            assert r1['smoothed'] is True and r1['raw'] == {k: r0[k] for k in ('left', 'right', 'offset')} and r1['matrix'] == r0['matrix']
            assert all(r1[k] == want[q][t][k] for k in ('left', 'right', 'offset', 'raw'))
            pics = []
            for o in (out0, out1):
                with Image.open(os.path.join(o, name, '%d.png' % t)) as im:
                    pics.append(np.asarray(im.convert('RGB')))
            assert pics[0].shape == (256, 512, 3) and np.array_equal(pics[0][:, :256], pics[1][:, :256])          # the crops are the same
            same_obj = open(os.path.join(out0, name, '%d.obj' % t)).read() == open(os.path.join(out1, name, '%d.obj' % t)).read()
            if t == 0:
                assert np.array_equal(pics[0], pics[1]) and same_obj and r1['left'] == r0['left']
            else:
                assert not same_obj and r1['left'] != r0['left']
    out2 = str(tmp_path / 'smooth15')
    assert P.main(common[:-3] + ['--workers', '2', '--out', out2, '--smooth', '--smooth_box', '--fps', '15', '--beta', '0']) == 2 * T
    want15 = P.predict(eng, seqs, first, ratio=0.8, stage=2, track=True, smooth={'fps': 15.0, 'beta': 0.0}, smooth_box={'fps': 15.0, 'beta': 0.0})
    with open(os.path.join(out2, 'a', '3.json')) as f:
        r = json.load(f)
    assert r['left'] == want15[0][3]['left'] and r['left'] != want[0][3]['left'] and r['smoothed'] is True
    assert r['box_smoothed'] is want15[0][3]['box_smoothed'] and r['matrix'] == want15[0][3]['matrix']
    capsys.readouterr()
    for flags in (['--smooth'], ['--smooth_box'], ['--beta', '0.1']):
        with pytest.raises(SystemExit) as e:
            P.main(['--model', ck, '--input', str(src), '--out', str(tmp_path / 'no')] + flags)
        assert e.value.code == 2
    assert 'need --track' in capsys.readouterr().err and not os.path.exists(str(tmp_path / 'no'))
    with pytest.raises(ValueError):
        P.predict(eng, seqs[0], None, smooth=True)


def matrices(mid_x, mid_y, L, size=256):
    s = (size / 2.0) / L
    z = np.zeros_like(s)
    return np.stack([s, z, s * (L - mid_x), z, s, s * (L - mid_y)], 1)


def test_smooth_matrices_alone():
    rng = np.random.default_rng(21)
    rows, frames = 3, 7
    mid = rng.uniform(200, 1800, (1, rows, 2)) + np.cumsum(rng.normal(size=(frames, rows, 2)) * 4, 0)
    L = rng.uniform(60, 400, (1, rows)) + np.cumsum(rng.normal(size=(frames, rows)) * 2, 0)
    ok = np.ones((frames, rows), np.int32)
    ok[3, 1] = ok[4, 1] = 0                                               # row 1 holds its box for two frames
    filt = SM.box_filter(rows)
    ref = OneEuroRef([(3, 1, 1.0)], rows)
    prev = None
    worst_f = worst_m = 0.0
    for t in range(frames):
        Mn = matrices(mid[t, :, 0], mid[t, :, 1], L[t])
        if prev is not None:
            Mn[ok[t] == 0] = prev[ok[t] == 0]                             # crop_matrices_from_meshes: the box holds, M_next = M_prev
        before = {k: filt.field(k).clone() for k in ('y1', 'y2', 'x1', 'x2', 'dxhat', 'jitter', 'age', 'count')}
        M, upd = SM.smooth_matrices(filt, torch.from_numpy(Mn).cuda(), torch.from_numpy(ok[t]).cuda(), 256)
        M, upd = M.cpu().numpy(), upd.cpu().numpy()
        # the restatement's chain: (mid_x, mid_y, L) out of M_next in float64, rounded to float32, through the filter
        Lb = 128.0 / Mn[:, 0]
        box = np.stack([Lb - Mn[:, 2] / Mn[:, 0], Lb - Mn[:, 5] / Mn[:, 0], Lb], 1).astype(np.float32)
        want, wupd = ref.step(box, ok[t])
        assert upd.tolist() == wupd.tolist() == [0 if not ok[t, b] else (2 if t == 0 else 1) for b in range(rows)]
        y = filt.field('y1').cpu().numpy()
        for b in range(rows):
            if upd[b] != 1:                                               # a first box, a held box: M_next itself, bit for bit
                assert np.array_equal(M[b].view(np.uint64), Mn[b].view(np.uint64)), (t, b)
            else:
                worst_f = max(worst_f, float(np.abs(y[b] - want[b]).max() / np.abs(box).max()))
                mine = matrices(y[b:b + 1, 0].astype(np.float64), y[b:b + 1, 1].astype(np.float64), y[b:b + 1, 2].astype(np.float64))[0]
                worst_m = max(worst_m, float(np.abs(M[b] - mine).max() / np.abs(mine).max()))
            if not ok[t, b]:                                              # a held box leaves the filter's values alone; only its age counts on
                for k in ('y1', 'y2', 'x1', 'x2', 'dxhat', 'jitter', 'count'):
                    assert torch.equal(filt.field(k)[b], before[k][b]), (t, b, k)
                assert int(filt.field('age')[b, 0]) == int(before['age'][b, 0]) + 1
        assert (M[:, 1] == 0).all() and (M[:, 3] == 0).all() and (M[:, 0] == M[:, 4]).all() and (M[:, 0] > 0).all() and np.isfinite(M).all()
        prev = M
    print('smooth_matrices: filter err %.3g (gate %.3g), matrix against the float64 formula %.3g' % (worst_f, GATE, worst_m))
    assert worst_f <= GATE and worst_m <= 1e-9


def test_smooth_box_in_predict(eng, video, plain):
    seqs, first = video
    recs = P.predict(eng, seqs, first, ratio=0.8, stage=2, track=True, smooth_box=True)
    flags = []
    for q in range(2):
        for t in range(T):
            r = recs[q][t]
            assert 'box_smoothed' not in plain[q][t] and 'smoothed' not in r and 'raw' not in r
            m = np.float64(r['matrix'])
            assert m[0, 1] == 0 and m[1, 0] == 0 and m[0, 0] == m[1, 1] and 2.0 ** -6 <= m[0, 0] <= 64.0 and np.isfinite(m).all() and r['valid'] is True
            if t < 2:                                                     # the given box, then the first tracked box: unchanged bit for bit
                assert r['matrix'] == plain[q][t]['matrix'] and r['box_smoothed'] is False
                assert r['left'] == plain[q][t]['left'] and r['tracked'] == plain[q][t]['tracked']
            if not r['tracked']:
                assert r['box_smoothed'] is False
                if t > 0:
                    assert r['matrix'] == recs[q][t - 1]['matrix']       # held
            flags.append(r['box_smoothed'])
    print('box_smoothed (sequence 0 frames 0..3, sequence 1 frames 0..3):', flags)
    # both together: the two filters do not share state
    both = P.predict(eng, seqs, first, ratio=0.8, stage=2, track=True, smooth=True, smooth_box=True)
    assert all(both[q][t]['matrix'] == recs[q][t]['matrix'] and both[q][t]['raw']['left'] == recs[q][t]['left'] for q in range(2) for t in range(T))
