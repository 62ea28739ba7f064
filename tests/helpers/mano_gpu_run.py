"""TEST INFRASTRUCTURE (GPU side of tests/helpers/mano_cases.py): runs case lists through the C ABI of the MANO kernels with guard rows after
every output buffer, parameters read in place from a `stride`-wide vector, and returns bit patterns.  Shared by tests/test_gpu_mano_sweep.py and
by the child process it starts per DIR_MANO_SPW value (python tests/helpers/mano_gpu_run.py OUT.npz)."""
import collections
import ctypes as C
import os
import sys

import numpy as np
import torch

_here = os.path.dirname(os.path.abspath(__file__))
if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(_here)))
if _here not in sys.path:
    sys.path.insert(0, _here)

from dir_amd import _capi, engine  # noqa: E402
import mano_cases as M  # noqa: E402

FILL = 3.0
BATCHES = (1, 2, 3, 5, 9, 17)
OUT_WIDTH = collections.OrderedDict([('verts', 2334), ('joints', 63), ('joint_uv', 42), ('mesh_uv', 1556)])
_PACKED = {}


def packed(kind, side, center, root_palm=False):
    key = (kind, side, center, root_palm)
    if key not in _PACKED:
        sd = {k: v.cuda() for k, v in M.state_dict(kind, side).items()}
        keep = []
        T = engine.pack_mano(sd, 'm', side, None if center < 0 else center, keep)
        T.root_palm = 1 if root_palm else 0
        _PACKED[key] = (T, keep, sd)
    return _PACKED[key][0]


def config(c):
    return (c.kind, c.side, c.center, c.root_palm)


def by_config(cases):
    out = collections.OrderedDict()
    for c in cases:
        out.setdefault(config(c), []).append(c)
    return out


def batches(cases, B):
    """the list cycled through batches of B: every case appears, at positions that change with B"""
    n = len(cases)
    return [[cases[(s + i) % n] for i in range(B)] for s in range(0, n, B)]


def launched():
    buf = C.create_string_buffer(1024)
    _capi.lib().dir_launch_log_get(buf, 1024)
    return [n for n in buf.value.decode().split(',') if n]


def _params(cases, stride):
    buf = torch.full((len(cases), stride), FILL)
    buf[:, :64] = torch.from_numpy(np.stack([c.para for c in cases]))
    return buf.cuda()


def _outputs(B, kinds=tuple(OUT_WIDTH)):
    out = {k: torch.full((B + 1, OUT_WIDTH[k]), FILL, device='cuda') for k in kinds}
    out['flags'] = torch.full((B + 1,), 77, dtype=torch.int32, device='cuda')
    return out


def _finish(outs, B, paras, befores, written):
    """guards and parameter buffers bit-unchanged; -> numpy bit patterns"""
    torch.cuda.synchronize()
    res = []
    for out, p, b0 in zip(outs, paras, befores):
        assert torch.equal(p.view(torch.int32), b0.view(torch.int32)), 'parameter buffer written'
        r = {}
        for k, t in out.items():
            fill = 77 if k == 'flags' else FILL
            if k in written:
                assert bool((t[B:] == fill).all()), 'guard row after %s written' % k
                r[k] = t[:B].cpu().numpy()
            else:
                assert bool((t == fill).all()), '%s written though its pointer was NULL' % k
        res.append(r)
    return res


def forward_single(cases, stride=64):
    """dir_mano_forward on cases of ONE config -> {kind: [B, width] float32, 'flags': [B]}"""
    B = len(cases)
    T = packed(*config(cases[0]))
    p = _params(cases, stride)
    before = p.clone()
    out = _outputs(B)
    base = p.data_ptr()
    _capi.lib().dir_launch_log_reset()
    rc = _capi.lib().dir_mano_forward(T, C.c_void_p(base), stride, C.c_void_p(base + 51 * 4), stride, C.c_void_p(base + 61 * 4), stride,
                                      _capi.ptr(out['verts']), _capi.ptr(out['joints']), _capi.ptr(out['joint_uv']), _capi.ptr(out['mesh_uv']),
                                      _capi.ptr(out['flags']), B, _capi.stream_ptr())
    _capi.check(rc, 'dir_mano_forward')
    names = launched()
    assert names == ['mano_forward_kernel'], names
    return _finish([out], B, [p], [before], set(out))[0]


def forward_pair(cases_lr, stride=64, projections=True):
    """dir_mano_forward_pair: cases_lr = two equally long lists, one config each.  projections=False: cam_lr, joint_uv_lr, mesh_uv_lr and
    flags_lr are all NULL."""
    B = len(cases_lr[0])
    Ts = (_capi.ManoTables * 2)(*[packed(*config(cs[0])) for cs in cases_lr])
    ps = [_params(cs, stride) for cs in cases_lr]
    befores = [p.clone() for p in ps]
    outs = [_outputs(B), _outputs(B)]
    P2 = C.c_void_p * 2
    arr = lambda k: P2(*[o[k].data_ptr() for o in outs])  # noqa: E731
    off = lambda o: P2(*[p.data_ptr() + 4 * o for p in ps])  # noqa: E731
    _capi.lib().dir_launch_log_reset()
    rc = _capi.lib().dir_mano_forward_pair(Ts, off(0), stride, off(51), stride, off(61) if projections else None, stride, arr('verts'), arr('joints'),
                                           arr('joint_uv') if projections else None, arr('mesh_uv') if projections else None,
                                           arr('flags') if projections else None, B, _capi.stream_ptr())
    _capi.check(rc, 'dir_mano_forward_pair')
    names = launched()
    assert names == ['mano_forward_kernel'], names
    return _finish(outs, B, ps, befores, set(outs[0]) if projections else {'verts', 'joints'})


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def spw_sweep():
    """what the DIR_MANO_SPW children and their parent both run: every 4-part config's cases at B = 1, 2, 3, 5, 9, 17 (B = 5 / 9: tails of one
    live sample in a group of 4 / of 2) and one pair call per B -> {label: array}"""
    res = {}
    cfgs = [(k, cs) for k, cs in by_config(M.forward_cases()).items() if not k[3] and k[2] not in (4, 8, 12, 16, 20)]
    for i, (key, cs) in enumerate(cfgs):
        for B in BATCHES:
            for n, batch in enumerate(batches(cs, B)):
                r = forward_single(batch, 64 if (i + B) % 2 else 70)
                for k, a in r.items():
                    res['s.%d.%d.%d.%s' % (i, B, n, k)] = a
    for j, B in enumerate(BATCHES):
        a, b = cfgs[j % len(cfgs)][1], cfgs[(j + 1) % len(cfgs)][1]
        r = forward_pair([batches(a, B)[0], batches(b, B)[0]])
        for h in (0, 1):
            for k, x in r[h].items():
                res['p.%d.%d.%s' % (B, h, k)] = x
    return res


if __name__ == '__main__':
    assert os.environ.get('DIR_MANO_SPW') in ('2', '4')
    torch.cuda.set_device(0)
    np.savez(sys.argv[1], **spw_sweep())
    print('OK')
