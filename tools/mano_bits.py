"""The bits of the four entry points that run the device-side MANO layer (csrc/mano_device.h): one SHA-256 per output tensor on fixed inputs.

  python tools/mano_bits.py [> listing]

The check for a change that must not move a bit of the layer: run it on a build of the parent commit and on the changed tree, with the same
compiler, and compare the two listings (`diff`).  Not a test: the hashes belong to one compiler version.  Inputs, all from tests/helpers:
  forward    mano_cases.forward_cases() per configuration through dir_mano_forward (small batches: four vertex parts; a root-palm table or a
             fingertip centre: one part) and neighbouring configurations through dir_mano_forward_pair
  backward   mano_cases.backward_cases() with cotangents() through dir_mano_backward_pair, one and two hands, and with cam / g_cam NULL
  fit        mano_fit_ref.problem: mesh / joints / uv at iters 0, 1, 10, both hands in one launch, root_palm off and on, and 5 + 5 iterations with the state
  smooth     para_smooth_ref.parity_case for both sides (passed-through and gap rows included), every frame's outputs and the final state
"""
import ctypes as C
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests', 'helpers'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import mano_cases as M  # noqa: E402
import mano_fit_ref as FR  # noqa: E402
import mano_gpu_run as G  # noqa: E402
import para_smooth_ref as PR  # noqa: E402

from dir_amd import _capi  # noqa: E402
from dir_amd import functional as F  # noqa: E402
from dir_amd.utils import mano_fit as MF  # noqa: E402
from dir_amd.utils import smooth as SM  # noqa: E402


def show(name, a):
    if isinstance(a, torch.Tensor):
        torch.cuda.synchronize()
        a = a.detach().contiguous().cpu().numpy()
    a = np.ascontiguousarray(a)
    print('%s  %-44s %s %s' % (hashlib.sha256(a.tobytes()).hexdigest(), name, a.dtype, list(a.shape)))


def dev(a, rows=None):
    if a is None:
        return None
    a = np.asarray(a)
    return torch.from_numpy(np.ascontiguousarray(a if rows is None else a[rows])).cuda()


def forward():
    cfgs = list(G.by_config(M.forward_cases()).items())
    for i, (key, cs) in enumerate(cfgs):
        tag = 'fwd.%s.%s.c%d%s' % (key[0], key[1], key[2], '.palm' if key[3] else '')
        for k, a in G.forward_single(cs, 64 if i % 2 else 70).items():
            show('%s.B%d.%s' % (tag, len(cs), k), a)
    for i in range(len(cfgs) - 1):
        a, b = cfgs[i][1], cfgs[i + 1][1]
        n = min(len(a), len(b))
        r = G.forward_pair([a[:n], b[:n]], projections=i % 3 != 2)
        for h in (0, 1):
            for k, x in r[h].items():
                show('fwdpair.%d.B%d.h%d.%s' % (i, n, h, k), x)


def backward():
    cfgs = list(G.by_config(M.backward_cases()).items())
    args = []
    for key, cs in cfgs:
        cots = [M.cotangents(c) for c in cs]
        para = dev(np.stack([c.para for c in cs]))
        g = {'g_' + k: dev(np.stack([c[k] for c in cots])) for k in M.KINDS}
        args.append((G.packed(*key), para, g))
    for i, ((key, cs), (T, para, g)) in enumerate(zip(cfgs, args)):
        tag = 'bwd.%s.%s.c%d.B%d' % (key[0], key[1], key[2], len(cs))
        show(tag + '.all', F.mano_backward([T], [para], **{k: [v] for k, v in g.items()})[0])
        show(tag + '.uv', F.mano_backward([T], [para], g_joint_uv=[g['g_joint_uv']], g_mesh_uv=[g['g_mesh_uv']])[0])
        # cam and g_cam NULL: the layer alone
        out = torch.zeros(len(cs), 64, device='cuda')
        P1 = C.c_void_p * 1
        _capi.check(_capi.lib().dir_mano_backward_pair((_capi.ManoTables * 1)(T), P1(para.data_ptr()), 64, P1(para.data_ptr() + 51 * 4), 64, None, 0,
                                                       P1(g['g_verts'].data_ptr()), P1(g['g_joints'].data_ptr()), None, None, P1(out.data_ptr()), 64,
                                                       P1(out.data_ptr() + 51 * 4), 64, None, 0, 1, len(cs), _capi.stream_ptr()), 'dir_mano_backward_pair')
        show(tag + '.nocam', out)
    for i in range(len(args) - 1):
        (Ta, pa, ga), (Tb, pb, gb) = args[i], args[i + 1]
        n = min(pa.shape[0], pb.shape[0])
        got = F.mano_backward([Ta, Tb], [pa[:n].contiguous(), pb[:n].contiguous()], **{k: [ga[k][:n].contiguous(), gb[k][:n].contiguous()] for k in ga})
        for h in (0, 1):
            show('bwdpair.%d.B%d.h%d' % (i, n, h), got[h])


FIT_FIELDS = ('para', 'verts', 'joints', 'joint_uv', 'mse_before', 'mse_after', 'status')


def fit_run(probs, iters, **kw):
    arg = lambda k: [dev(getattr(p, k)) for p in probs]  # noqa: E731
    tabs = [G.packed(FR.KIND, p.side, p.center, p.root_palm) for p in probs]
    return MF.fit_mano(tabs, kw.pop('init', None) or arg('init'), arg('verts'), arg('joints'), arg('joints_conf'), arg('joint_uv'), arg('uv_conf'), iters=iters,
                       lr=dict(zip(MF.GROUPS, probs[0].lr)), weights=probs[0].weights, **kw)


def fit():
    for config in ('mesh', 'joints', 'uv'):
        for palm in (False, True):
            probs = [FR.problem(config, 3, s, root_palm=palm) for s in ('left', 'right')]
            tag = 'fit.%s%s' % (config, '.palm' if palm else '')
            for iters in (0, 1, 10):
                r = fit_run(probs, iters)
                for h in (0, 1):
                    for k in FIT_FIELDS:
                        show('%s.it%d.h%d.%s' % (tag, iters, h, k), getattr(r, k)[h])
            first = fit_run(probs, 5, state=True)
            second = fit_run(probs, 5, state=first.state, init=[t.clone() for t in first.para], anchor=[dev(p.init) for p in probs])
            for h in (0, 1):
                for k in FIT_FIELDS:
                    show('%s.it5+5.h%d.%s' % (tag, h, k), getattr(second, k)[h])
                show('%s.it5+5.h%d.state' % (tag, h), second.state[h])


def smooth():
    sides = ('left', 'right')
    frames = [PR.parity_case(s) for s in sides]
    sm = SM.ParameterSmoother([G.packed(PR.KIND, s, PR.CENTER, False) for s in sides], PR.SEQS, **PR.CASE_OPTS)
    keys = ('smoothed', 'verts', 'joints', 'joints_px', 'updated')
    outs = [{k: [] for k in keys} for _ in sides]
    for t in range(PR.FRAMES):
        para = [dev(f[t]['para']) for f in frames]
        cam = [dev(f[t]['cam_px']) for f in frames]
        raws = [tuple(dev(f[t]['raw'][k]) for k in ('verts', 'joints', 'joints_px')) for f in frames]
        for o, r in zip(outs, sm.launch(para, cam, dev(frames[0][t]['valid']), raws)):
            for k in keys:
                o[k].append(r[k].clone())
    for h, s in enumerate(sides):
        for k in keys:
            show('smooth.%s.%s' % (s, k), torch.stack(outs[h][k]))
        for name in ('measures', 'y1', 'y2', 'x1', 'x2', 'prev', 'vel', 'n_shape', 'age', 'run', 'count'):
            show('smooth.%s.state.%s' % (s, name), sm.field(name)[h])


if __name__ == '__main__':
    torch.cuda.set_device(0)
    forward()
    backward()
    fit()
    smooth()
