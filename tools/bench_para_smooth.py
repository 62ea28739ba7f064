"""Measures the parameter-space smoothing (dir_mano_para_smooth_step, apps.predict --smooth --smooth_space para) on the GPU.  No gates: it
prints what it finds.

  python tools/bench_para_smooth.py kernels [--b 32 256] [--rounds 20] [--reps 20]
      HIP events around --reps back-to-back calls (divided by --reps), one process, warmed, the variants alternating round by round; median
      and range per variant with the host's time to enqueue one call beside it.  B sequences x 2 hands, as
        para_smooth   dir_mano_para_smooth_step in its steady state (every row updates and counts its measures; raw streams given)
        mano_pair     dir_mano_forward_pair alone at the same B: the work the new launch contains
        one_euro      dir_one_euro_step on the PredictionSmoother layout (9 segments, F = 4887): the point-space smoother it stands beside
        composed      the composition it replaces: dir_one_euro_step on a [B,128] parameter tensor, then dir_mano_forward_pair
        copy          a device-to-device copy of the bytes the new launch moves: per (sequence, hand) the state row in and out, the outputs
                      and the raw streams
  python tools/bench_para_smooth.py app [--model CKPT] [--sequences 8] [--frames 24] [--rounds 2] [--parent TREE]
      apps.predict --track on a generated folder of sequences (tools/bench_smooth.py's), with no flag, with --smooth and with --smooth
      --smooth_space para, alternating, after a warm run of each: the command's own rate line.  --parent TREE: a built checkout of the parent
      commit whose unflagged loop joins the alternation in a child process.
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import bench_smooth as BS  # noqa: E402  (puts the measured tree on sys.path)

import numpy as np  # noqa: E402


def packed_tables(side, center=9):
    import torch

    from dir_amd import engine, synth
    sd = {'m.' + k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in synth.mano_buffers(side, 1234).items()}
    keep = []
    return engine.pack_mano(sd, 'm', side, center, keep), (keep, sd)


def kernels_at(B, opt):
    import torch

    from dir_amd import _capi
    from dir_amd.utils import smooth as SM
    L, P, stream = _capi.lib(), _capi.ptr, _capi.stream_ptr()
    rng = np.random.default_rng(0)
    tabs, keep = zip(*[packed_tables(s) for s in SM.SIDES])
    sm = SM.ParameterSmoother(list(tabs), B)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()  # noqa: E731
    para = []
    for _ in range(2):
        p = rng.normal(0, 0.3, (B, 64))
        p[:, 0:6] = np.array([1.0, 0, 0, 0, 1.0, 0]) + rng.normal(0, 0.1, (B, 6))
        p[:, 61:64] = (4.0, 0.0, 0.0)
        para.append(dev(p))
    cam = [dev(np.tile([200.0, 300.0, 250.0], (B, 1))) for _ in range(2)]
    raw = [(dev(rng.normal(0, 0.05, (B, 778, 3))), dev(rng.normal(0, 0.05, (B, 21, 3))), dev(rng.normal(300, 50, (B, 21, 2)))) for _ in range(2)]
    out = [{'smoothed': torch.empty(B, 64, device='cuda'), 'verts': torch.empty(B, 778, 3, device='cuda'), 'joints': torch.empty(B, 21, 3, device='cuda'),
            'joints_px': torch.empty(B, 21, 2, device='cuda'), 'updated': torch.empty(B, dtype=torch.int32, device='cuda')} for _ in range(2)]
    hs = (_capi.ManoParaSmoothHand * 2)()
    for h in range(2):
        x = hs[h]
        x.para, x.cam_px, (x.raw_verts, x.raw_joints, x.raw_joints_px) = para[h].data_ptr(), cam[h].data_ptr(), [t.data_ptr() for t in raw[h]]
        x.smoothed, x.verts, x.joints, x.joints_px, x.updated = (out[h][k].data_ptr() for k in ('smoothed', 'verts', 'joints', 'joints_px', 'updated'))
        x.state = sm.state[h].data_ptr()
    P2 = ctypes.c_void_p * 2
    off = lambda o: P2(*[p.data_ptr() + 4 * o for p in para])  # noqa: E731
    arr = lambda k: P2(*[o[k].data_ptr() for o in out])  # noqa: E731
    uv = [torch.empty(B, 21, 2, device='cuda') for _ in range(2)]
    pair_args = (sm.tables, off(0), 64, off(51), 64, off(61), 64, arr('verts'), arr('joints'), P2(*[u.data_ptr() for u in uv]), None, None, B, stream)
    point = SM.OneEuro([(p, d, v) for _, p, d, v in SM.STREAMS], B)
    xs = dev(rng.normal(size=(B, point.F)))
    ys, upd = torch.empty_like(xs), torch.empty(B, dtype=torch.int32, device='cuda')
    point_args = (P(xs), None, B, point._segs, point.S, point.fps, point.min_cutoff, point.beta, point.d_cutoff, point.max_gap, P(point.state), P(ys), P(upd), stream)
    par = SM.OneEuro([(128, 1, 1.0)], B)
    xp = torch.cat(para, 1).contiguous()
    yp, updp = torch.empty_like(xp), torch.empty(B, dtype=torch.int32, device='cuda')
    par_args = (P(xp), None, B, par._segs, par.S, par.fps, par.min_cutoff, par.beta, par.d_cutoff, par.max_gap, P(par.state), P(yp), P(updp), stream)
    nbytes = 2 * B * (2 * sm.row_bytes + 4 * (64 + 2439 + 1) + 4 * 2439 + 4 * 67)
    pool = torch.empty(nbytes, dtype=torch.uint8, device='cuda')

    def composed():
        _capi.check(L.dir_one_euro_step(*par_args), 'dir_one_euro_step')
        _capi.check(L.dir_mano_forward_pair(*pair_args), 'dir_mano_forward_pair')
    variants = {'para_smooth': lambda: _capi.check(L.dir_mano_para_smooth_step(sm.tables, hs, None, ctypes.byref(sm._opts), 2, B, stream), 'dir_mano_para_smooth_step'),
                'mano_pair': lambda: _capi.check(L.dir_mano_forward_pair(*pair_args), 'dir_mano_forward_pair'),
                'one_euro': lambda: _capi.check(L.dir_one_euro_step(*point_args), 'dir_one_euro_step'),
                'composed': composed,
                'copy': lambda: pool[nbytes // 2:].copy_(pool[:nbytes // 2])}
    for fn in variants.values():                                                         # warm; after three calls every row counts its measures
        for _ in range(4):
            fn()
    torch.cuda.synchronize()
    assert out[0]['updated'].cpu().tolist() == [1] * B and out[1]['updated'].cpu().tolist() == [1] * B and upd.cpu().tolist() == [1] * B
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times, hosts = {k: [] for k in variants}, {k: [] for k in variants}
    for _ in range(opt.rounds):
        for k, fn in variants.items():
            t, h = BS.timed(fn, e0, e1, opt.reps)
            times[k].append(t)
            hosts[k].append(h)
    print('B = %d sequences x 2 hands, %d rounds of %d calls, %d bytes moved per para_smooth call' % (B, opt.rounds, opt.reps, nbytes))
    res = {}
    for k in variants:
        t = np.array(times[k])
        res[k] = {'us_median': float(np.median(t)), 'us_min': float(t.min()), 'us_max': float(t.max()), 'host_enqueue_us': float(np.median(hosts[k]))}
        print('%-12s %8.1f us  (%.1f .. %.1f; host enqueue %.1f us)' % (k, res[k]['us_median'], t.min(), t.max(), res[k]['host_enqueue_us']))
    res['bytes'] = nbytes
    return res


def kernels(opt):
    print(json.dumps({'bench_para_smooth_kernels': {str(B): kernels_at(B, opt) for B in opt.b}}))


def app(opt):
    with tempfile.TemporaryDirectory() as tmp:
        src = BS.make_video(tmp, opt.sequences, opt.frames)
        model = opt.model or BS.synthetic_model(tmp)
        argv = ['--model', model, '--input', src, '--boxes', os.path.join(tmp, 'boxes.json'), '--track', '--bs', str(opt.sequences)]
        print('%d sequences of %d frames (640 x 480), one forward per frame over all sequences' % (opt.sequences, opt.frames))
        for k in range(opt.rounds):
            for name, flags in (('plain', []), ('--smooth', ['--smooth']), ('para', ['--smooth', '--smooth_space', 'para'])):
                for line in BS.run_predict(argv, os.path.join(tmp, 'out_%s_%d' % (name.strip('-'), k)), flags, 2):
                    print('%-10s %s' % (name, line))
            if opt.parent:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), 'app-child', '--argv', json.dumps(argv), '--out', os.path.join(tmp, 'out_parent_%d' % k)],
                                   env=dict(os.environ, DIR_BENCH_TREE=os.path.abspath(opt.parent)), capture_output=True, text=True, timeout=600)
                if r.returncode != 0:
                    raise RuntimeError('the parent tree failed (%d):\n%s' % (r.returncode, r.stderr[-2000:]))
                for line in r.stdout.splitlines():
                    if line.startswith('RATE '):
                        print('%-10s %s' % ('parent', line[5:]))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    sub = ap.add_subparsers(dest='cmd', required=True)
    k = sub.add_parser('kernels')
    k.add_argument('--b', type=int, nargs='+', default=[32, 256])
    k.add_argument('--rounds', type=int, default=20)
    k.add_argument('--reps', type=int, default=20)
    a = sub.add_parser('app')
    a.add_argument('--model', default=None)
    a.add_argument('--sequences', type=int, default=8)
    a.add_argument('--frames', type=int, default=24)
    a.add_argument('--rounds', type=int, default=2)
    a.add_argument('--parent', type=str, default=None)
    c = sub.add_parser('app-child')
    c.add_argument('--argv', required=True)
    c.add_argument('--out', required=True)
    opt = ap.parse_args()
    {'kernels': kernels, 'app': app, 'app-child': BS.app_child}[opt.cmd](opt)


if __name__ == '__main__':
    main()
