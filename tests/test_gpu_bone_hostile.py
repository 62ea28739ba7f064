"""GPU: the bone path -- dir_bone_proj_forward, dir_bone_fusion_prepare / _forward in its four precisions, dir_bone_proj_backward and
dir_bone_fusion_backward -- on the hostile joints of tests/helpers/bone_cases.py (pixels at exactly `distance`, rounding-decided diagonals,
zero-length bones, joints on the image corner / outside / at uv = +-50, bones on every strip seam, NaN and +-Inf joints), one bone and one
tap at a time.  The reference is the float32 restatement oracle.tokens.bone_proj (tests/test_bone_cases_ref.py pins the fixtures to it) and
oracle.spatial_grad.bone_proj_backward.

One-hot fusion weights: for a tap t, output channel n < 240 selects hand-bone n // 6 and feature channel c_n = (n % 6) * 11
(W[n, t, hb * 64 + c_n] = 1, everything else 0, scale 1, shift 0), so

    y[b, y, x, n] = img[b, hb * 64 + c_n, y + ky - 1, x + kx - 1]      (0 outside the image; channels 240..255 exactly 0)

is a pure shift of one channel of the bone image.  Support: (y != 0) equals the shifted restatement mask exactly, per bone and per tap, in
every mode -- no tolerance, no band.  Values, relative to F = max |feat|:

    fp32              2^-22 F        one rounding of each product's sum on the exact matrix cores against two in the restatement
    split precision   5e-6 F         the project's own gate for that kernel
    bf16              4 * 2^-9 F     pixel weight, G and output each rounded to nearest; positive terms, nothing cancels; one unit of margin
    f16               4 * 2^-11 F    the same argument at f16 precision

Measured on the MI355X (F = 4.6929), one-hot fusion, largest |y - restatement| over every sample and tap:
    (S, B)     bf16          f16           fp32          split precision
    (16, 3)    3.733e-3 F    5.326e-4 F    5.080e-8 F    1.524e-7 F
    (32, 2)    4.153e-3 F    5.373e-4 F    5.080e-8 F    1.524e-7 F
    (32, 5)    4.153e-3 F    5.373e-4 F    5.080e-8 F    1.524e-7 F
    (64, 1)    3.987e-3 F    5.411e-4 F    refused by the guard (the halo patch of a 128-pixel strip does not fit)
    bound      7.812e-3 F    1.953e-3 F    2.384e-7 F    5.000e-6 F
S = 64 in the 16-bit modes (a patch of 396 rows against the limit of 400) is accepted and right: support and values hold on every sample.
Materialised map, largest |out - restatement|: fp32 0 (bit-identical) at S = 16, 32, 64; bf16 1.547e-2 / 1.519e-2 / 7.81e-3 (tolerance 2e-2);
f16 1.716e-3 / 1.939e-3 / 9.77e-4 (tolerance 2^-11 F = 2.291e-3).
Dense weights, of the output maximum, S = 16 / 32: fp32 factorised 4.78e-7 / 4.56e-7 against materialised 3.35e-6 / 2.52e-6; split precision
3.62e-7 / 5.05e-7; bf16 |factorised - materialised| 5.91e-3 / 3.79e-3, |factorised - fp32| 3.69e-3 / 3.60e-3; f16 7.38e-4 / 4.74e-4 and
5.79e-4 / 4.02e-4.
Backward, per sample of its maximum: bone_proj S = 16 g emb 2.15e-7, g uv 5.93e-7; S = 32 g emb 4.75e-7, g uv 2.06e-6; factorised fusion S = 16
y 7.33e-7, g weight 2.26e-7, g emb 4.27e-7, g uv 2.66e-6.
"""
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'helpers'))
import bone_cases as BC  # noqa: E402

from dir_amd import _capi  # noqa: E402
from dir_amd import functional as Fn  # noqa: E402
from dir_amd.train import spatial as TSP  # noqa: E402
from oracle import tokens as OT  # noqa: E402
from oracle.spatial_grad import bone_proj_backward  # noqa: E402

pytestmark = pytest.mark.gpu

# mode -> (exact_f32, output dtype, split precision)
MODES = {'bf16': (0, torch.bfloat16, False), 'f16': (2, torch.float16, False), 'fp32': (1, torch.float32, False), 'split': (1, torch.float32, True)}
VALUE_BOUND = {'fp32': 2.0 ** -22, 'split': 5e-6, 'bf16': 4 * 2.0 ** -9, 'f16': 4 * 2.0 ** -11}      # x F
NSEL = 240


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Cases:
    """the samples of one S with their restatement, shared by every test of that S and never modified"""

    def __init__(self, S):
        self.S, self.dist = S, BC.distance(S)
        self.names, self.uv = BC.samples(S, 2)                            # [n, 2, 21, 2]
        self.n = len(self.names)
        self.feat = BC.features(self.n)                                   # [n, 42, 64]
        self.F = float(np.abs(self.feat).max())
        sel = list(BC.CSEL)
        img, mask = [], []
        for h in range(2):
            i, m = OT.bone_proj(self.uv[:, h], self.feat[:, 21 * h:21 * h + 21][:, :, sel], S, self.dist, return_mask=True)
            img.append(i)                                                 # [n, 20 * 6, S, S]: channel bone * 6 + k
            mask.append(m)                                                # [n, S, S, 20]
        self.img6 = np.concatenate(img, 1)                                # [n, 240, S, S]: channel n = (hand * 20 + bone) * 6 + k
        self.mask = np.concatenate(mask, 3)                               # [n, S, S, 40]
        assert np.isfinite(self.img6).all()
        assert np.array_equal(self.img6.transpose(0, 2, 3, 1) != 0, np.repeat(self.mask, 6, 3))
        pad = np.zeros((self.n, S + 2, S + 2, NSEL), np.float32)
        pad[:, 1:-1, 1:-1] = self.img6.transpose(0, 2, 3, 1)
        self.ref_pad = dev(pad)                                           # NHWC with the convolution's zero border
        self.d_uv, self.d_feat = dev(self.uv), dev(self.feat)
        self._full = None

    def idx(self, name):
        return self.names.index(name)

    def full(self):
        """the whole 64-channel restatement [n, 2560, S, S] (S <= 32 only: the materialised and dense-weight tests)"""
        if self._full is None:
            self._full = np.concatenate([OT.bone_proj(self.uv[:, h], self.feat[:, 21 * h:21 * h + 21], self.S, self.dist) for h in range(2)], 1)
        return self._full


_CASES = {}


@pytest.fixture(scope='module')
def cases():
    def get(S):
        if S not in _CASES:
            _CASES[S] = Cases(S)
        return _CASES[S]
    yield get
    _CASES.clear()


@pytest.fixture(scope='module')
def onehot():
    """w_g [9][40][64][256] of tap t (include/dir_hip.h: dir_bone_fusion_params.w_g), made once per tap"""
    made = {}

    def get(tap):
        if tap not in made:
            w = torch.zeros(9, 40, 64, 256, device='cuda')
            n = torch.arange(NSEL, device='cuda')
            w[tap, n // 6, (n % 6) * 11, n] = 1.0
            made[tap] = w
        return made[tap]
    yield get
    made.clear()


def g_scale_for(amax):
    """the engine's calibration: the power of two that puts the largest |G| into [2^9, 2^10)"""
    return 2.0 ** (10 - math.frexp(amax)[1])


class Fusion:
    """dir_bone_fusion_prepare + dir_bone_fusion_forward into channels [32, 288) of a 320-channel buffer filled with a sentinel"""

    def __init__(self, w_g, scale, shift):
        self.L = _capi.lib()
        self.w_g, self.scale, self.shift = w_g, scale, shift

    def run(self, mode, uv, emb, S, dist, relu, g_scale=None):
        exact, odt, split = MODES[mode]
        B = emb.shape[0]
        uv_l, uv_r = uv[:, 0].contiguous(), uv[:, 1].contiguous()
        P = _capi.BoneFusionParams(self.w_g.data_ptr(), self.scale.data_ptr(), self.shift.data_ptr(), exact, float(g_scale) if split else 0.0)
        scratch = torch.empty(self.L.dir_bone_fusion_scratch_bytes(B), device='cuda', dtype=torch.uint8)
        y = torch.full((B, S, S, 320), 7.0, device='cuda', dtype=odt)
        _capi.check(self.L.dir_bone_fusion_prepare(P, _capi.ptr(emb), _capi.ptr(scratch), B, _capi.stream_ptr()), 'bone_fusion_prepare')
        _capi.check(self.L.dir_bone_fusion_forward(P, _capi.ptr(uv_l), _capi.ptr(uv_r), _capi.ptr(scratch), _capi.ptr(y), B, S, float(dist), 320, 32,
                                                   int(relu), _capi.stream_ptr()), 'bone_fusion_forward')
        torch.cuda.synchronize()
        assert float(y[..., :32].float().min()) == 7.0 and float(y[..., :32].float().max()) == 7.0, 'wrote below the channel slice'
        assert float(y[..., 288:].float().min()) == 7.0 and float(y[..., 288:].float().max()) == 7.0, 'wrote above the channel slice'
        return y[..., 32:288]


def where(bad, rows, names, tap):
    """the first offending element of a [B, S, S, 240] boolean tensor, in words"""
    b, y, x, n = [int(v) for v in torch.nonzero(bad)[0]]
    hb = n // 6
    return 'sample %s (row %d), %s hand bone %d, feature channel %d, tap (ky %d, kx %d), output pixel (y %d, x %d); %d elements differ' % (
        names[rows[b]], b, 'right' if hb >= 20 else 'left', hb % 20, (n % 6) * 11, tap // 3, tap % 3, y, x, int(bad.sum()))


def chunks(n, B):
    """every sample in a batch of B: consecutive rows, the last batch wrapping round"""
    return [[(i + k) % n for k in range(B)] for i in range(0, n, B)]


@pytest.mark.parametrize('S,B', [(16, 3), (32, 2), (32, 5), (64, 1)])
def test_one_hot_fusion_support_and_values_per_bone_and_tap(cases, onehot, S, B):
    """every sample, every tap, both hands, every mode; ReLU off and on (all values are >= 0: the two must be bit-identical)"""
    cs = cases(S)
    one, zero = torch.ones(256, device='cuda'), torch.zeros(256, device='cuda')
    modes = [m for m in MODES if S <= 32 or MODES[m][0] != 1]             # S = 64: the 16-bit modes (the fp32 kernels refuse it, see the guard test)
    worst = {m: 0.0 for m in modes}
    gs = g_scale_for(cs.F)                                                # one-hot weights: G holds feature values, |G| <= F
    for rows in chunks(cs.n, B):
        uv, emb = cs.d_uv[rows].contiguous(), cs.d_feat[rows].contiguous()
        for tap in range(9):
            ky, kx = tap // 3, tap % 3
            fu = Fusion(onehot(tap), one, zero)
            want = cs.ref_pad[rows][:, ky:ky + S, kx:kx + S]             # img[y + ky - 1, x + kx - 1]
            for mode in modes:
                y = fu.run(mode, uv, emb, S, cs.dist, False, gs)
                got = y[..., :NSEL].float()
                assert bool(torch.isfinite(y.float()).all()), (mode, 'NaN / Inf in y')
                assert float(y[..., NSEL:].float().abs().max()) == 0.0, (mode, 'channels 240..255 must be exactly 0')
                bad = (got != 0) != (want != 0)
                assert not bool(bad.any()), 'support differs from the restatement, S=%d B=%d mode %s: %s' % (S, B, mode, where(bad, rows, cs.names, tap))
                err = (got - want).abs()
                e = float(err.max()) / cs.F
                worst[mode] = max(worst[mode], e)
                assert e <= VALUE_BOUND[mode], 'value %.3e F > %.3e F, S=%d B=%d mode %s: %s' % (
                    e, VALUE_BOUND[mode], S, B, mode, where(err == err.max(), rows, cs.names, tap))
                y_relu = fu.run(mode, uv, emb, S, cs.dist, True, gs)
                assert torch.equal(y, y_relu), (mode, tap, 'ReLU changed non-negative values')
    for mode in modes:
        print('MEASURED: one-hot fusion S=%d B=%d %-5s max |y - restatement| = %.3e F  (bound %.3e F, F = %.4f)' % (S, B, mode, worst[mode], VALUE_BOUND[mode], cs.F))


@pytest.mark.parametrize('S', [16, 32])
def test_one_hot_fusion_poisoned_sample_is_isolated(cases, onehot, S):
    """[ties, poison, edges] against [ties, ties, edges]: the clean rows bit-identical, the poisoned row's untouched bones bit-identical to
    `ties`, its poisoned bones exactly 0, no NaN / Inf anywhere (the poisoned row carries the features of `ties` in both batches)"""
    cs = cases(S)
    one, zero = torch.ones(256, device='cuda'), torch.zeros(256, device='cuda')
    rows_p = [cs.idx('ties'), cs.idx('poison'), cs.idx('edges')]
    rows_c = [cs.idx('ties'), cs.idx('ties'), cs.idx('edges')]
    poisoned = dev(np.repeat(BC.poisoned_bones().reshape(40), 6))         # [240] bool
    gs = g_scale_for(cs.F)
    for tap in range(9):
        fu = Fusion(onehot(tap), one, zero)
        for mode in MODES:
            yp = fu.run(mode, cs.d_uv[rows_p].contiguous(), cs.d_feat[rows_c].contiguous(), S, cs.dist, False, gs)      # the features of `ties`
            yc = fu.run(mode, cs.d_uv[rows_c].contiguous(), cs.d_feat[rows_c].contiguous(), S, cs.dist, False, gs)
            assert bool(torch.isfinite(yp.float()).all()), (mode, tap)
            assert torch.equal(yp[0], yc[0]) and torch.equal(yp[2], yc[2]), (mode, tap, 'a clean row changed with a poisoned neighbour')
            assert torch.equal(yp[1][..., :NSEL][..., ~poisoned], yc[1][..., :NSEL][..., ~poisoned]), (mode, tap)
            assert float(yp[1][..., :NSEL][..., poisoned].float().abs().max()) == 0.0, (mode, tap, 'a poisoned bone rasterised to something')
            assert float(yc[1][..., :NSEL][..., poisoned].float().abs().max()) > 0.0


def test_fusion_guards():
    """S = 64 with exact_f32 = 1 (either fp32 kernel): refused by name, nothing launched"""
    L = _capi.lib()
    B, S = 1, 64
    z = torch.zeros(9 * 40 * 64 * 256, device='cuda')
    uv = torch.zeros(B, 21, 2, device='cuda')
    scratch = torch.zeros(L.dir_bone_fusion_scratch_bytes(B), device='cuda', dtype=torch.uint8)
    for g_scale in (0.0, 128.0):
        P = _capi.BoneFusionParams(z.data_ptr(), z.data_ptr(), z.data_ptr(), 1, g_scale)
        y = torch.full((B, S, S, 256), 7.0, device='cuda')
        rc = L.dir_bone_fusion_forward(P, _capi.ptr(uv), _capi.ptr(uv), _capi.ptr(scratch), _capi.ptr(y), B, S, 4.0, 256, 0, 1, _capi.stream_ptr())
        assert rc != 0 and b'dir_bone_fusion_forward' in L.dir_last_error()
        torch.cuda.synchronize()
        assert float(y.min()) == 7.0 and float(y.max()) == 7.0


def bone_proj(cs, rows, dt, want_vis=True, want_bbox=True, want_out=True):
    tdt = {_capi.DT_F32: torch.float32, _capi.DT_BF16: torch.bfloat16, _capi.DT_F16: torch.float16}[dt]
    B, S = len(rows), cs.S
    uv, emb = cs.d_uv[rows], cs.d_feat[rows].contiguous()
    uv_l, uv_r = uv[:, 0].contiguous(), uv[:, 1].contiguous()
    out = torch.full((B, S, S, 2560), 9.0, device='cuda', dtype=tdt) if want_out else None
    vis = torch.full((B, 1280, S, S), 9.0, device='cuda') if want_vis else None
    bbox = torch.full((B, 40, 4), -77, device='cuda', dtype=torch.int32) if want_bbox else None
    _capi.check(_capi.lib().dir_bone_proj_forward(_capi.ptr(uv_l), _capi.ptr(uv_r), _capi.ptr(emb), _capi.ptr(out), _capi.ptr(vis), _capi.ptr(bbox), B, S,
                                                  float(cs.dist), dt, _capi.stream_ptr()), 'bone_proj')
    torch.cuda.synchronize()
    return out, vis, bbox


@pytest.mark.parametrize('S', [16, 32, 64])
def test_materialised_bone_map_mask_values_and_boxes(cases, S):
    """dir_bone_proj_forward on every sample in every storage type, with vis and bbox: the mask is the restatement's on all 64 channels, the
    values sit within test_bone_proj_vs_reference's tolerances (fp32 1e-6, bf16 2e-2; f16: 2^-11 F, one rounding to nearest of a value <= F),
    the boxes contain every non-zero and are empty for poisoned, zero-length and off-image bones; dir_conv2d_sparse_forward on that map is
    bit-identical to the dense convolution"""
    cs = cases(S)
    rows = list(range(cs.n))
    B = cs.n
    mask = dev(cs.mask)                                                   # [n, S, S, 40]
    sel = torch.tensor(BC.CSEL, device='cuda')
    ref_sel = cs.ref_pad[:, 1:-1, 1:-1].reshape(B, S, S, 40, 6)
    ref_full = dev(cs.full().transpose(0, 2, 3, 1)).reshape(B, S, S, 40, 64) if S <= 32 else None
    must_be_empty = np.zeros((cs.n, 40), bool)
    must_be_empty[cs.idx('poison')] = BC.poisoned_bones().reshape(40)
    for i in (cs.idx('ties'), cs.idx('poison')):
        must_be_empty[i, 3::4] = True                                     # zero length
    for hand, k in BC.EDGES_OFF_IMAGE:
        must_be_empty[cs.idx('edges'), hand * 20 + k] = True
    assert not cs.mask[must_be_empty[:, None, None, :].repeat(S, 1).repeat(S, 2)].any()
    vis_ref = None
    for dt, tol in ((_capi.DT_F32, 1e-6), (_capi.DT_BF16, 2e-2), (_capi.DT_F16, 2.0 ** -11 * cs.F)):
        out, vis, bbox = bone_proj(cs, rows, dt)
        o = out.float().reshape(B, S, S, 40, 64)
        assert bool(torch.isfinite(o).all()) and bool(torch.isfinite(vis).all())
        bad = (o != 0) != mask[..., None]
        assert not bool(bad.any()), 'bone_proj mask differs (S=%d dtype %d) at (sample, y, x, hand-bone, channel) %s' % (S, dt, torch.nonzero(bad)[0].tolist())
        e = float((o[..., sel] - ref_sel).abs().max()) if ref_full is None else float((o - ref_full).abs().max())
        print('MEASURED: bone_proj S=%d dtype %d max |out - restatement| = %.3e (tolerance %.3e)' % (S, dt, e, tol))
        assert e < tol, (S, dt, e)
        # vis = left + right, fp32 whatever the storage type
        v = vis.reshape(B, 20, 64, S, S).permute(0, 3, 4, 1, 2)           # [B, S, S, 20, 64]
        if ref_full is None:
            ev = float((v[..., sel] - (ref_sel[..., :20, :] + ref_sel[..., 20:, :])).abs().max())
        else:
            ev = float((v - (ref_full[..., :20, :] + ref_full[..., 20:, :])).abs().max())
        assert ev < 2e-6, (S, dt, ev)
        if vis_ref is None:
            vis_ref = vis
            _, vis_only, _ = bone_proj(cs, rows, dt, want_bbox=False, want_out=False)      # the proj_feat-only launch
            assert torch.equal(vis_only, vis)
        else:
            assert torch.equal(vis, vis_ref)
        # boxes
        bb = bbox.cpu().numpy()
        assert (bb != -77).all()
        nz = (o != 0).any(-1).cpu().numpy()                               # [B, S, S, 40]
        for b in range(B):
            for g in range(40):
                ys, xs = np.nonzero(nz[b, :, :, g])
                y0, y1, x0, x1 = bb[b, g]
                if len(ys):
                    assert y0 <= ys.min() and ys.max() <= y1 and x0 <= xs.min() and xs.max() <= x1, (S, dt, cs.names[b], g)
                if must_be_empty[b, g]:
                    assert y0 > y1 or x0 > x1, 'box of an empty bone is not empty: S=%d dtype %d sample %s hand-bone %d: %s' % (S, dt, cs.names[b], g, bb[b, g])
        if S <= 32 and dt != _capi.DT_F16:                                # the sparse convolution, in the storage types the existing bbox test runs it in
            w = (torch.randn(256, 3, 3, 2560, device='cuda') * 0.02).to(out.dtype)
            shift = torch.randn(256, device='cuda')
            dense = Fn.conv2d_nhwc(out, w, 1, 1, shift=shift, relu=True)
            d = _capi.ConvDesc(B, S, S, 2560, 2560, 0, 256, 256, 0, 0, 0, 3, 3, 1, 1, Fn._dt(out), Fn._dt(out), 1, 0, 0)
            sparse = torch.empty_like(dense)
            _capi.check(_capi.lib().dir_conv2d_sparse_forward(d, _capi.ptr(out), _capi.ptr(w), None, _capi.ptr(shift), None, _capi.ptr(sparse), _capi.ptr(bbox),
                                                              _capi.stream_ptr()), 'sparse')
            assert torch.equal(dense, sparse), 'sparse-K conv differs from dense (S=%d, dtype %d)' % (S, dt)


@pytest.mark.parametrize('S', [16, 32])
def test_dense_weights_on_hostile_joints_factorised_vs_materialised(cases, S):
    """random weights (each mode's own rounding of them), every sample in one batch: the factorised result against the materialised GPU path
    (dir_bone_proj_forward + the implicit-GEMM convolution in the same storage type) under the gates of the existing tests: 1.5e-2 of the
    output maximum in the 16-bit modes; in fp32, twice the materialised path's own error + 1e-6, both errors taken against the float64 sum of
    the SAME fp32 products (the restatement's bone map times the weights, one float64 matrix product per sample on the GPU); the split
    precision kernel also under its 5e-6.  And f16 is no further from the fp32 result than bf16 is."""
    cs = cases(S)
    rows = list(range(cs.n))
    B = cs.n
    rng = np.random.default_rng(900 + S)
    w = dev((rng.standard_normal((256, 2560, 3, 3)) * 0.02).astype(np.float32))
    scale = dev((1 + 0.1 * rng.standard_normal(256)).astype(np.float32))
    shift = dev((0.1 * rng.standard_normal(256)).astype(np.float32))
    uv, emb = cs.d_uv, cs.d_feat

    def factorised(mode, wm, g_scale=None):
        return Fusion(TSP.fusion_w_g(wm), scale, shift).run(mode, uv, emb, S, cs.dist, True, g_scale).float()

    def materialised(dt, wm):
        out, _, _ = bone_proj(cs, rows, dt, want_vis=False, want_bbox=False)
        return Fn.conv2d_nhwc(out, wm.permute(0, 2, 3, 1).contiguous().to(out.dtype), 1, 1, scale=scale, shift=shift, relu=True).float()

    # float64 sum of the fp32 operands
    img = dev(cs.full())                                                  # [n, 2560, S, S], the restatement
    w64 = w.double().reshape(256, 2560 * 9)
    ref = torch.empty(B, S, S, 256, device='cuda', dtype=torch.float64)
    for b in range(B):
        cols = torch.nn.functional.unfold(img[b:b + 1].double(), 3, padding=1)[0]      # [2560 * 9, S * S], rows (c, ky, kx)
        ref[b] = (w64 @ cols).t().reshape(S, S, 256)
    ref = torch.relu(ref * scale.double() + shift.double())
    sc = float(ref.abs().max())
    y32, m32 = factorised('fp32', w), materialised(_capi.DT_F32, w)
    e_f, e_m = float((y32 - ref).abs().max()), float((m32 - ref).abs().max())
    print('MEASURED: dense hostile S=%d fp32: factorised %.2e, materialised %.2e of the output maximum' % (S, e_f / sc, e_m / sc))
    assert bool(torch.isfinite(y32).all())
    assert e_f <= 2.0 * e_m + 1e-6 * sc, (e_f, e_m, sc)
    # split precision, calibrated as the engine does (largest |G| -> [2^9, 2^10))
    L = _capi.lib()
    scratch = torch.empty(L.dir_bone_fusion_scratch_bytes(B), device='cuda', dtype=torch.uint8)
    wg = TSP.fusion_w_g(w)
    P = _capi.BoneFusionParams(wg.data_ptr(), scale.data_ptr(), shift.data_ptr(), 1, 0.0)
    _capi.check(L.dir_bone_fusion_prepare(P, _capi.ptr(emb), _capi.ptr(scratch), B, _capi.stream_ptr()), 'prepare')
    amax = float(scratch.view(torch.float32)[:B * 9 * 40 * 256 * 2].abs().max())
    y3 = factorised('split', w, g_scale_for(amax))
    e_3 = float((y3 - ref).abs().max())
    print('MEASURED: dense hostile S=%d split precision: %.2e of the output maximum' % (S, e_3 / sc))
    assert e_3 <= 2.0 * e_m + 1e-6 * sc and e_3 <= 5e-6 * sc, (e_3, e_m, sc)
    dist32 = {}
    for mode, dt, tdt in (('bf16', _capi.DT_BF16, torch.bfloat16), ('f16', _capi.DT_F16, torch.float16)):
        wm = w.to(tdt).float()                                            # this mode's weights
        yf, ym = factorised(mode, wm), materialised(dt, wm)
        assert bool(torch.isfinite(yf).all())
        e = float((yf - ym).abs().max())
        dist32[mode] = float((yf - y32).abs().max())
        print('MEASURED: dense hostile S=%d %s: |factorised - materialised| %.2e, |factorised - fp32| %.2e of the output maximum' % (S, mode, e / sc, dist32[mode] / sc))
        assert e <= 1.5e-2 * sc, (mode, e, sc)
    assert dist32['f16'] <= dist32['bf16'], dist32


def rel(got, ref):
    """largest error of any sample relative to THAT sample's maximum (no sample hides behind another's larger gradient); tensors without a
    batch axis (the weight gradient) as a whole"""
    got, ref = got.cpu().numpy().astype(np.float64), np.asarray(ref, np.float64)
    if ref.ndim == 4 and ref.shape[0] == 256:
        return float(np.abs(got - ref).max() / np.abs(ref).max())
    ax = tuple(range(1, ref.ndim))
    return float((np.abs(got - ref).max(ax) / np.abs(ref).max(ax)).max())


@pytest.mark.parametrize('S', [16, 32])
def test_bone_proj_backward_on_hostile_joints(cases, S):
    """dir_bone_proj_backward on ties, borders and plain against oracle.spatial_grad.bone_proj_backward (float64, the float32 restatement's
    mask): 1e-5 of each tensor's maximum per sample, 1e-4 for g uv; two calls bit-identical; a poisoned neighbour changes no other row"""
    cs = cases(S)
    rows = [cs.idx(nm) for nm in ('ties', 'edges', 'seams', 'plain0', 'plain1')]
    B = len(rows)
    rng = np.random.default_rng(300 + S)
    g_img = rng.standard_normal((B, 2560, S, S)).astype(np.float32)
    uv, feat = cs.uv[rows], cs.feat[rows]
    ref = [bone_proj_backward(uv[:, h], feat[:, 21 * h:21 * h + 21], g_img[:, 1280 * h:1280 * h + 1280], S, cs.dist) for h in range(2)]
    assert all(np.isfinite(r[0]).all() and np.isfinite(r[1]).all() for r in ref)
    d_g = dev(g_img).permute(0, 2, 3, 1).contiguous()
    d_uv, d_emb = cs.d_uv[rows], cs.d_feat[rows].contiguous()
    args = (d_uv[:, 0].contiguous(), d_uv[:, 1].contiguous(), d_emb, d_g, S, cs.dist)
    g_emb, gul, gur = TSP.bone_proj_bwd(*args)
    torch.cuda.synchronize()
    e_f = rel(g_emb, np.concatenate([ref[0][1], ref[1][1]], 1))
    e_u = max(rel(gul, ref[0][0]), rel(gur, ref[1][0]))
    print('MEASURED: bone_proj backward hostile S=%d: g emb %.2e, g uv %.2e of the maximum' % (S, e_f, e_u))
    assert e_f < 1e-5 and e_u < 1e-4, (e_f, e_u)
    again = TSP.bone_proj_bwd(*args)
    assert all(torch.equal(a, b) for a, b in zip((g_emb, gul, gur), again))
    # [ties, poison, edges] against [ties, ties, edges]
    outs = []
    clean = [cs.idx(nm) for nm in ('ties', 'ties', 'edges')]
    for names in (('ties', 'poison', 'edges'), ('ties', 'ties', 'edges')):
        u = cs.d_uv[[cs.idx(nm) for nm in names]]
        outs.append(TSP.bone_proj_bwd(u[:, 0].contiguous(), u[:, 1].contiguous(), cs.d_feat[clean].contiguous(), d_g[:3].contiguous(), S, cs.dist))
    torch.cuda.synchronize()
    for a, b in zip(*outs):
        assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])


def test_bone_fusion_backward_on_hostile_joints(cases):
    """dir_bone_fusion_prepare / _forward (exact fp32) + dir_bone_fusion_backward at S = 16 on ties, borders and plain against the float64
    composition of the existing test (restatement bone map, float64 convolution differentiated by autograd, the float64 bone_proj backward):
    1e-5 of each tensor's maximum, 1e-4 for g uv; two calls bit-identical; with a poisoned neighbour the other rows' g emb and g uv keep
    their bits (the weight gradient sums over the batch and is only checked without poison)"""
    S = 16
    cs = cases(S)
    rows = [cs.idx(nm) for nm in ('ties', 'edges', 'seams', 'plain0')]
    B = len(rows)
    rng = np.random.default_rng(41)
    W = (rng.standard_normal((256, 2560, 3, 3)) * 0.02).astype(np.float32)
    bias = rng.standard_normal(256).astype(np.float32)
    gy = rng.standard_normal((B, S, S, 256)).astype(np.float32)
    uv, feat = cs.uv[rows], cs.feat[rows]
    ti = torch.from_numpy(cs.full()[rows].astype(np.float64)).requires_grad_(True)
    tw = torch.from_numpy(W.astype(np.float64)).requires_grad_(True)
    y_ref = torch.nn.functional.conv2d(ti, tw, torch.from_numpy(bias.astype(np.float64)), padding=1)
    y_ref.backward(torch.from_numpy(gy.astype(np.float64)).permute(0, 3, 1, 2))
    g_img, g_w_ref = ti.grad.numpy(), tw.grad.numpy()
    gu, gf = zip(*[bone_proj_backward(uv[:, h], feat[:, 21 * h:21 * h + 21], g_img[:, 1280 * h:1280 * h + 1280], S, cs.dist) for h in range(2)])
    w_g, d_bias, d_gy = TSP.fusion_w_g(dev(W)), dev(bias), dev(gy)

    def run(r, r_feat):
        u = cs.d_uv[r]
        y, ctx = TSP.bone_fusion_fwd(u[:, 0].contiguous(), u[:, 1].contiguous(), cs.d_feat[r_feat].contiguous(), w_g, d_bias, S, cs.dist)
        return y, ctx, TSP.bone_fusion_bwd(ctx, d_gy[:len(r)].contiguous())

    y, ctx, (g_w_g, g_emb, gul, gur) = run(rows, rows)
    torch.cuda.synchronize()
    e_y = rel(y, y_ref.detach().permute(0, 2, 3, 1).numpy())
    e_w = rel(TSP.fusion_w_g_grad_to_oihw(g_w_g), g_w_ref)
    e_f = rel(g_emb, np.concatenate(gf, 1))
    e_u = max(rel(gul, gu[0]), rel(gur, gu[1]))
    print('MEASURED: factorised fusion hostile S=16 vs float64: y %.2e, g weight %.2e, g emb %.2e, g uv %.2e' % (e_y, e_w, e_f, e_u))
    assert e_y < 1e-5 and e_w < 1e-5 and e_f < 1e-5 and e_u < 1e-4, (e_y, e_w, e_f, e_u)
    again = TSP.bone_fusion_bwd(ctx, d_gy)
    assert all(torch.equal(a, b) for a, b in zip((g_w_g, g_emb, gul, gur), again))
    clean = [cs.idx(nm) for nm in ('ties', 'ties', 'edges')]
    outs = [run([cs.idx(nm) for nm in names], clean) for names in (('ties', 'poison', 'edges'), ('ties', 'ties', 'edges'))]
    torch.cuda.synchronize()
    assert bool(torch.isfinite(outs[0][0]).all())                         # the forward of the poisoned batch
    assert torch.equal(outs[0][0][0], outs[1][0][0]) and torch.equal(outs[0][0][2], outs[1][0][2])
    for a, b in zip(outs[0][2][1:], outs[1][2][1:]):                      # g emb, g uv left, g uv right
        assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2])
