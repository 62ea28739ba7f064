"""CPU: the restatement of the One-Euro rule (tests/helpers/one_euro_ref.py), the inverse crop maps, and the host side of the C ABI.

  closed forms   a constant input returns itself exactly; with beta = 0 the filter is a first-order one: its step response is
                 1 - (1 - a)^t with a = 1 / (1 + fps / (2 pi fc)); the jitter of c t^2 is 2 |c| raw
  the paper      for D = 1 the restatement equals a literal transcription of the pseudo-code of Casiez, Roussel, Vogel (CHI 2012), written
                 here independently, to 1e-12; for D = 3 rotating the input rotates the output
  gaps           after k unusable frames the state's age is k + 1: while age <= max_gap the next update uses dt = (k + 1) / fps; beyond,
                 the filter starts again (the rule compares the AGE with max_gap, so max_gap - 1 missing frames is the longest gap bridged)
  crop maps      crop_camera and from_frame_pixels invert frame_camera and to_frame_pixels to 1e-9 px on random axis-aligned matrices
  C ABI          dir_one_euro_step checks its arguments before any launch; dir_one_euro_state_bytes is a pure host function"""
import ctypes
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'helpers'))
from one_euro_ref import OneEuroRef, alpha  # noqa: E402


def run(ref, xs, valid=None):
    ys, ups = [], []
    for t, x in enumerate(xs):
        y, u = ref.step(x, None if valid is None else valid[t])
        ys.append(y)
        ups.append(u)
    return np.stack(ys), np.stack(ups)


def test_constant_input_returns_itself_exactly():
    rng = np.random.default_rng(0)
    x = rng.normal(size=(2, 5 * 3 + 4 * 2)) * 100
    ref = OneEuroRef([(5, 3, 1000.0), (4, 2, 1.0)], 2)
    ys, ups = run(ref, [x] * 6)
    assert all(np.array_equal(y, x) for y in ys)
    assert ups.tolist() == [[2, 2]] + [[1, 1]] * 5 and ref.count.tolist() == [4, 4] and not ref.jitter.any()


def test_beta_zero_is_a_first_order_filter():
    fps, fc, T = 30.0, 1.5, 40
    a = 1.0 / (1.0 + fps / (2.0 * math.pi * fc))
    ref = OneEuroRef([(1, 1, 1.0)], 1, fps=fps, min_cutoff=fc, beta=0.0)
    xs = [np.zeros((1, 1))] + [np.ones((1, 1))] * T                       # the step arrives after the initialising frame
    ys, _ = run(ref, xs)
    want = np.array([0.0] + [1.0 - (1.0 - a) ** t for t in range(1, T + 1)])
    assert np.abs(ys[:, 0, 0] - want).max() < 1e-14
    assert abs(alpha(fc, 1.0 / fps) - a) < 1e-16


class PaperFilter(object):
    """Casiez et al. 2012, the pseudo-code of the paper, transcribed literally for one scalar: LowPassFilter with hatxprev, and
    OneEuroFilter with its two low-pass filters; rate is fixed"""

    def __init__(self, rate, mincutoff, beta, dcutoff):
        self.rate, self.mincutoff, self.beta, self.dcutoff = rate, mincutoff, beta, dcutoff
        self.first = True
        self.x_hatxprev = self.dx_hatxprev = None

    def _alpha(self, cutoff):
        tau = 1.0 / (2 * math.pi * cutoff)
        te = 1.0 / self.rate
        return 1.0 / (1.0 + tau / te)

    def filter(self, x):
        if self.first:
            self.first = False
            dx = 0.0
            self.dx_hatxprev = dx                     # LowPassFilter: the first value initialises hatxprev
            self.x_hatxprev = x
            return x
        dx = (x - self.x_hatxprev) * self.rate
        a = self._alpha(self.dcutoff)
        edx = a * dx + (1 - a) * self.dx_hatxprev
        self.dx_hatxprev = edx
        cutoff = self.mincutoff + self.beta * abs(edx)
        a = self._alpha(cutoff)
        out = a * x + (1 - a) * self.x_hatxprev
        self.x_hatxprev = out
        return out


def test_scalar_equals_the_papers_pseudo_code():
    rng = np.random.default_rng(1)
    T, N = 60, 7
    xs = np.cumsum(rng.normal(size=(T, 1, N)), 0) + rng.normal(size=(T, 1, N)) * 0.1
    for beta in (0.007, 0.5):
        ref = OneEuroRef([(N, 1, 1.0)], 1, fps=60.0, min_cutoff=1.0, beta=beta, d_cutoff=1.0)
        ys, _ = run(ref, xs)
        for n in range(N):
            f = PaperFilter(60.0, 1.0, beta, 1.0)
            want = np.array([f.filter(float(v)) for v in xs[:, 0, n]])
            assert np.abs(ys[:, 0, n] - want).max() < 1e-12, (beta, n)


def test_rotating_the_input_rotates_the_output():
    rng = np.random.default_rng(2)
    T, N = 30, 9
    xs = np.cumsum(rng.normal(size=(T, 1, N, 3)), 0)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    ya, _ = run(OneEuroRef([(N, 3, 2.0)], 1, beta=0.3), xs.reshape(T, 1, -1))
    yb, _ = run(OneEuroRef([(N, 3, 2.0)], 1, beta=0.3), (xs @ q.T).reshape(T, 1, -1))
    assert np.abs(ya.reshape(T, 1, N, 3) @ q.T - yb.reshape(T, 1, N, 3)).max() < 1e-12 * np.abs(xs).max()
    # a per-component cutoff would not pass: the speed is the point's, not the component's
    assert np.abs(ya - xs.reshape(T, 1, -1)).max() > 1e-3


def test_gaps():
    fps, fc = 30.0, 1.0
    for k in (1, 2, 3):                                                   # k unusable frames: age k + 1 <= max_gap 4: dt = (k + 1) / fps
        ref = OneEuroRef([(1, 1, 1.0)], 1, fps=fps, min_cutoff=fc, beta=0.0, max_gap=4)
        xs = [np.zeros((1, 1))] + [np.full((1, 1), np.nan)] * k + [np.ones((1, 1))]
        ys, ups = run(ref, xs)
        assert ups[:, 0].tolist() == [2] + [0] * k + [1]
        assert np.isnan(ys[1:1 + k]).all()                                # passed through
        assert abs(ys[-1, 0, 0] - alpha(fc, (k + 1) / fps)) < 1e-15 and ref.age[0] == 1 and ref.run[0] == 1
    # the same through `valid`, and an age beyond max_gap (3 missing frames: age 4 > 3) initialises again
    ref = OneEuroRef([(1, 1, 1.0)], 1, fps=fps, min_cutoff=fc, beta=0.0, max_gap=3)
    xs = [np.zeros((1, 1))] + [np.full((1, 1), 5.0)] * 3 + [np.ones((1, 1))]
    ys, ups = run(ref, xs, valid=[[1], [0], [0], [0], [1]])
    assert ups[:, 0].tolist() == [2, 0, 0, 0, 2] and ys[1, 0, 0] == 5.0 and ys[-1, 0, 0] == 1.0 and ref.dxhat[0, 0] == 0.0
    # a row that was never initialised does not age
    ref = OneEuroRef([(1, 1, 1.0)], 1, max_gap=3)
    ref.step(np.full((1, 1), np.inf))
    assert ref.age[0] == 0 and ref.run[0] == 0


def test_jitter_of_a_quadratic_ramp():
    c, T = -0.37, 12
    xs = [np.array([[c * t * t, 3.0 + c * t * t, c * t * t, 0.0]]) for t in range(T)]
    ref = OneEuroRef([(2, 1, 1.0), (1, 2, 1.0)], 2)
    run(ref, xs)
    m = ref.mean_jitter()
    assert ref.count.tolist() == [T - 2, 0]                               # run >= 3 from the third frame on; row 1 never ran
    assert abs(m[0, 0, 0] - 2 * abs(c)) < 1e-12 and abs(m[0, 1, 0] - 2 * abs(c)) < 1e-12      # the D = 2 point moves along one axis
    assert 0 < m[0, 0, 1] < 2 * abs(c)                                    # the filtered ramp lags, its second difference is smaller
    # an unusable frame interrupts the run: two more frames pass before the jitter counts again
    ref = OneEuroRef([(1, 1, 1.0)], 1)
    run(ref, [np.array([[float(t * t)]]) for t in range(4)] + [np.array([[np.nan]])] + [np.array([[float(t * t)]]) for t in range(5, 9)])
    assert ref.count[0] == 2 + 2


def test_crop_maps_invert_their_counterparts():
    import torch
    from dir_amd.utils import crop as CR
    rng = np.random.default_rng(3)
    B, size = 64, 256
    s = np.exp(rng.uniform(np.log(1 / 16), np.log(16), B))
    M = torch.from_numpy(np.stack([s, np.zeros(B), rng.uniform(-3000, 3000, B), np.zeros(B), s, rng.uniform(-3000, 3000, B)], 1))
    uv = torch.from_numpy(rng.uniform(-1.5, 1.5, (B, 21, 2)).astype(np.float32))
    px = CR.to_frame_pixels(uv, M, size)                                  # float32
    back = CR.from_frame_pixels(px, M, size)
    assert back.dtype == torch.float64
    again = ((back + 1.0) * size / 2.0 - M[:, None, (2, 5)]) / M[:, None, 0:1]      # to_frame_pixels' formula, not rounded
    assert float((again - px.double()).abs().max()) < 1e-9
    assert torch.equal(CR.to_frame_pixels(back, M, size), px)
    proj = torch.from_numpy(np.concatenate([rng.uniform(2, 20, (B, 1)), rng.uniform(-1, 1, (B, 2))], 1).astype(np.float32))
    sc, tr = CR.frame_camera(proj, M, size)
    p = CR.crop_camera(sc, tr, M, size)
    assert p.dtype == torch.float64 and tuple(p.shape) == (B, 3)
    sc2 = p[:, 0] * size / 2.0 / M[:, 0]
    tr2 = ((p[:, 1:3] + 1.0) * size / 2.0 - M[:, (2, 5)]) / M[:, 0:1]
    # a camera scale is pixels per metre: thousands; 1e-9 px at the 0.1 m a hand spans
    assert float((sc2 - sc.double()).abs().max()) * 0.1 < 1e-9 and float((tr2 - tr.double()).abs().max()) < 1e-9
    a, b = CR.frame_camera(p, M, size)
    assert torch.equal(a, sc) and torch.equal(b, tr)


def test_entry_point_checks_its_arguments_before_any_launch():
    import torch  # noqa: F401
    from dir_amd import _capi
    L = _capi.lib()
    one = ctypes.c_void_p(16)
    Seg = _capi.OneEuroSegment

    def call(x=one, B=1, segs=((3, 1, 1.0),), S=None, fps=30.0, mc=1.0, beta=0.007, dc=1.0, gap=30, state=one, y=one, upd=one):
        arr = (Seg * max(1, len(segs)))(*[Seg(*g) for g in segs])
        return L.dir_one_euro_step(x, None, B, arr if segs is not None else None, len(segs) if S is None else S, fps, mc, beta, dc, gap, state, y, upd, None)

    def bad(rc, word):
        assert rc == -1 and word in L.dir_last_error(), (rc, L.dir_last_error())
    bad(call(x=None), b'null pointer')
    bad(call(state=None), b'null pointer')
    bad(call(y=None), b'null pointer')
    bad(call(upd=None), b'null pointer')
    bad(L.dir_one_euro_step(one, None, 1, None, 1, 30.0, 1.0, 0.0, 1.0, 30, one, one, one, None), b'null pointer')
    bad(call(B=0), b'B 0')
    bad(call(B=4097), b'B 4097')
    bad(call(segs=((1, 1, 1.0),) * 17), b'17 segments')
    bad(call(S=0), b'0 segments')
    bad(call(segs=((3, 5, 1.0),)), b'D 5')
    bad(call(segs=((3, 0, 1.0),)), b'D 0')
    bad(call(segs=((4096, 4, 1.0), (1, 1, 1.0))), b'over the limit')
    bad(call(segs=((0, 1, 1.0),)), b'points')
    bad(call(fps=0.0), b'rate')
    bad(call(fps=float('nan')), b'rate')
    bad(call(mc=0.0), b'rate')
    bad(call(dc=-1.0), b'rate')
    bad(call(beta=-0.1), b'beta')
    bad(call(gap=0), b'max_gap')
    bad(call(y=ctypes.c_void_p(18)), b'aligned')


def test_state_bytes_is_a_pure_host_function():
    import torch  # noqa: F401
    from dir_amd import _capi
    L = _capi.lib()
    off = (ctypes.c_longlong * 9)()
    assert L.dir_one_euro_state_bytes(0, 1, None) == -1 and L.dir_one_euro_state_bytes(1, 0, None) == -1
    assert L.dir_one_euro_state_bytes(16385, 1, None) == -1 and L.dir_one_euro_state_bytes(1, 17, None) == -1 and L.dir_one_euro_state_bytes(-3, 1, None) == -1
    prev = 0
    for F in (1, 2, 3, 4, 5, 922, 4887, 16384):
        n = L.dir_one_euro_state_bytes(F, 4, off)
        o = list(off)
        assert n >= prev and n % 16 == 0 and n >= 5 * 4 * F + 4 * 16 + 12
        assert n > prev or F <= 4                                         # strictly monotone beyond the padding of a row
        prev = n
        # jitter (double [S,2]) first, five float32 [F] planes, three int32; nothing overlaps, everything inside the row
        assert o[0] == 0 and o[1] == 64 and [b - a for a, b in zip(o[1:6], o[2:7])] == [4 * F] * 5 and o[7] == o[6] + 4 and o[8] == o[7] + 4 and o[8] + 4 <= n
    assert L.dir_one_euro_state_bytes(922, 16, None) > L.dir_one_euro_state_bytes(922, 4, None)


def test_python_wrapper_checks_and_state_views():
    """OneEuro's host side without a device: the argument checks, and the views of a row-major state"""
    import pytest
    import torch
    from dir_amd.utils import smooth as SM
    f = SM.OneEuro([(300, 3, 1000.0), (5, 2, 1.0), (3, 1, 1.0), (1, 3, 1000.0)], 3, device='cpu')
    assert f.F == 916 and f.S == 4 and f.max_gap == 30 and tuple(f.state.shape) == (3, f.row_bytes)
    assert tuple(f.field('y1').shape) == (3, 916) and f.field('y1').dtype == torch.float32
    assert tuple(f.field('jitter').shape) == (3, 4, 2) and f.field('jitter').dtype == torch.float64 and tuple(f.field('age').shape) == (3, 1)
    f.field('x2')[1, 7] = 2.5
    f.field('count')[2, 0] = 9
    raw = f.state.numpy()
    assert raw[1, f.offsets['x2'] + 28:f.offsets['x2'] + 32].view(np.float32)[0] == 2.5 and raw[2, f.offsets['count']:f.offsets['count'] + 4].view(np.int32)[0] == 9
    j = f.jitter()
    assert j['frames'].tolist() == [0, 0, 9] and j['raw'].shape == (3, 4) and np.isnan(j['raw'][0]).all() and not j['raw'][2].any()
    f.reset([2])
    assert f.jitter()['frames'].tolist() == [0, 0, 0] and f.field('x2')[1, 7] == 2.5
    f.reset()
    assert not f.state.any()
    for bad in ([], [(1, 1, 1.0)] * 17, [(3, 5, 1.0)], [(0, 1, 1.0)], [(4096, 4, 1.0), (1, 1, 1.0)]):
        with pytest.raises(ValueError):
            SM.OneEuro(bad, 1, device='cpu')
    for kw in ({'fps': 0}, {'min_cutoff': 0}, {'beta': -1}, {'d_cutoff': 0}, {'max_gap': 0}):
        with pytest.raises(ValueError):
            SM.OneEuro([(1, 1, 1.0)], 1, device='cpu', **kw)
    with pytest.raises(ValueError):
        SM.OneEuro([(1, 1, 1.0)], 0, device='cpu')
    assert sum(p * d for _, p, d, _ in SM.STREAMS) == 4887 and len(SM.STREAMS) == 9
