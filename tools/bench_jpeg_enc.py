"""Measurements of the JPEG encode path (reported, not gated).  HIP events, one process, warmed, variants alternating, outputs allocated once.

    python tools/bench_jpeg_enc.py kernels [--rounds 20 --calls 20]
        B = 256 frames of 256 x 256: dir_jpeg_encode_records against a device copy of the bytes it moves (frames read + records written),
        dir_jpeg_decode_records alone and the round trip (encode + decode)
    python tools/bench_jpeg_enc.py host [--frames 64 --rounds 5]
        us per frame, one core: dir_jpeg_encode_record (Huffman coding of a record) against Pillow's full encode of the same frames
    python tools/bench_jpeg_enc.py app [--images 1024 --runs 3] [--parent DIR]
        render_split on a generated split with and without --gpu_encode, each run a child process of its own, alternating; --parent: a built
        checkout of the parent commit, whose (unflagged) tool runs in the same alternation.  Then the tool's own loop once per mode with a
        clock around every step of the main process and inside every worker task (what bounds the tool), and the phases of one batch of
        256, each timed alone in this process: annotation reads, GT MANO + render, device-to-host copy, the encode, the transfer to a
        pool worker (pickle round trip of a chunk), the file writes and the start of the pool.

Every figure is printed with its run count and spread (min / median / max); nothing is estimated."""
import argparse
import io
import json
import os
import pickle
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests', 'helpers'))


def spread(xs):
    xs = sorted(xs)
    return 'min %.4g / median %.4g / max %.4g (n = %d)' % (xs[0], xs[len(xs) // 2], xs[-1], len(xs))


def rendered_like_frames(B, seed=0):
    """dense/-like frames: black background, two blobs with hard edges and smooth colour inside"""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:256, 0:256].astype(np.float32)
    out = np.zeros((B, 256, 256, 3), np.uint8)
    for b in range(B):
        for cx, cy in (rng.uniform(60, 110, 2), rng.uniform(140, 200, 2)):
            inside = (xx - cx) ** 2 + (yy - cy) ** 2 < rng.uniform(30, 55) ** 2
            col = np.stack([127 + 120 * np.sin(xx / (13.0 + c + b % 7)) * np.cos(yy / (9.0 + c)) for c in range(3)], -1)
            out[b][inside] = np.clip(col[inside], 0, 255).astype(np.uint8)
    return out


def timed(fn, calls):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls * 1e3                              # us per call


def kernels(opt):
    import torch
    from dir_amd.apps import jpeg as AJ
    B = 256
    frames = torch.from_numpy(rendered_like_frames(B)).cuda()
    enc = AJ.RecordEncoder(B, 256, 95)
    recs = torch.zeros(B, enc.record_bytes, dtype=torch.uint8, device='cuda')
    out = torch.zeros_like(frames)
    dec = AJ.RecordDecoder(B, enc.record_bytes, 256)
    moved = frames.numel() + recs.numel()
    src, dst = torch.zeros(moved // 2, dtype=torch.uint8, device='cuda'), torch.zeros(moved // 2, dtype=torch.uint8, device='cuda')
    variants = {'encode': lambda: enc(frames, recs), 'copy of the same bytes': lambda: dst.copy_(src), 'decode': lambda: dec(recs, out),
                'round trip': lambda: (enc(frames, recs), dec(recs, out))}
    for fn in variants.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    assert torch.equal(out, AJ.jpeg_round_trip(frames))
    us = {k: [] for k in variants}
    for _ in range(opt.rounds):
        for k, fn in variants.items():
            us[k].append(timed(fn, opt.calls))
    print('kernels: B = %d frames of 256 x 256, quality 95; %d rounds of %d calls, variants alternating; us per call' % (B, opt.rounds, opt.calls))
    for k in variants:
        med = sorted(us[k])[len(us[k]) // 2]
        extra = ''
        if k in ('encode', 'copy of the same bytes'):
            extra = '   %.1f MB read + written -> %.0f GB/s at the median' % (moved / 1e6, moved / (med * 1e-6) / 1e9)
        print('  %-24s %s   %.2f us per frame%s' % (k, spread(us[k]), med / B, extra))
    med = {k: sorted(v)[len(v) // 2] for k, v in us.items()}
    print('  encode / copy = %.2f' % (med['encode'] / med['copy of the same bytes']))


def host(opt):
    from PIL import Image
    from dir_amd.apps import jpeg as AJ
    import jpeg_enc_ref as R
    frames = rendered_like_frames(opt.frames)
    noise = np.clip(np.random.RandomState(1).normal(128, 50, frames.shape), 0, 255).astype(np.uint8)
    for name, fr in (('rendered-like frames', frames), ('noise frames', noise)):
        recs = [R.encode_record(f, 95) for f in fr]
        lib = AJ.host_lib()
        assert AJ.record_to_bytes(recs[0]) == R.encode_file(fr[0], 95)
        t_rec, t_pil, sizes = [], [], []
        for _ in range(opt.rounds):
            t0 = time.perf_counter()
            for r in recs:
                sizes.append(len(AJ.record_to_bytes(r)))
            t1 = time.perf_counter()
            for f in fr:
                Image.fromarray(np.ascontiguousarray(f[:, :, ::-1])).save(io.BytesIO(), format='JPEG', quality=95, subsampling=2)
            t2 = time.perf_counter()
            t_rec.append((t1 - t0) / len(fr) * 1e6)
            t_pil.append((t2 - t1) / len(fr) * 1e6)
        del lib
        print('host, %s (%d frames of 256 x 256, quality 95, mean file %.0f bytes), one core, us per frame:' % (name, len(fr), np.mean(sizes)))
        print('  dir_jpeg_encode_record (record -> file bytes, through record_to_bytes)   %s' % spread(t_rec))
        print('  Pillow full encode (frame -> file bytes)                                %s' % spread(t_pil))


def _child(tree, root, ckpt, dense, flags):
    env = dict(os.environ, PYTHONPATH=tree)
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, '-m', 'dir_amd.apps.render_split', '--save_path', root, '--model', ckpt, '--dense_color', dense, '--bs', '256'] + flags,
                       cwd=tree, env=env, capture_output=True, text=True, timeout=900)
    wall = time.perf_counter() - t0
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    tail = r.stdout.strip().splitlines()[-1]
    return float(tail.split(':')[-1].split('images/s')[0]), wall


def _timed_call(name, args):
    """in a pool worker: one task of render_split's (by name) -> (its result, seconds it took)"""
    from dir_amd.apps import render_split as RS
    t0 = time.perf_counter()
    out = getattr(RS, name)(*args)
    return out, time.perf_counter() - t0


def profiled_run(root, state, table, gpu_encode, bs=256):
    """render_split's own loop (same calls, same pool, same bounds) with a clock around every step of the main process and inside every
    worker task -> seconds per step, summed over the run, and the rate over the second half of the batches (every worker has imported its
    modules by then: a spawned worker pays about a second for that the first time it gets a task of either kind).  The render is followed by a synchronise here, so that its time is not charged
    to the device-to-host copy behind it."""
    import multiprocessing as mp
    import torch
    from dir_amd import _capi
    from dir_amd.apps import dataset as DS
    from dir_amd.apps import render_split as RS
    from dir_amd.apps.jpeg import RecordEncoder
    from dir_amd.utils import vis_utils as V
    dev, split = 'cuda', 'train'
    workers = RS.default_workers()
    mano = DS.gt_layers_from_checkpoint(state, dev)
    faces = torch.from_numpy(V.faces_from_layers(mano)).to(dev)
    colors = torch.from_numpy(V.load_dense_colors(table)).to(dev)
    n = len(DS.InterHandSplit(root, split))
    ws = torch.empty(int(_capi.lib().dir_render_workspace_bytes(bs)), dtype=torch.uint8, device=dev)
    batches = [list(range(s0, min(n, s0 + bs))) for s0 in range(0, n, bs)]
    chunk = max(1, -(-bs // workers))
    enc = RecordEncoder(2 * bs, DS.IMG_SIZE, quality=95, channel_order='bgr')
    recs = torch.empty(2 * bs, enc.record_bytes, dtype=torch.uint8, device=dev)
    write = '_write_records' if gpu_encode else '_write'
    T = {k: 0.0 for k in ('pool start', 'wait for annotations', 'GT MANO + render (+ GPU encode)', 'device-to-host', 'wait for a free slot (workers behind)',
                          'submit to the pool (pickling)', 'drain at the end', 'worker seconds: annotation reads', 'worker seconds: encode + write')}
    clock = time.perf_counter
    stamps = []                                                            # when each batch was handed to the pool

    def take(res, key):
        out, sec = res.get()
        T[key] += sec
        return out
    t_all = clock()
    with mp.get_context('spawn').Pool(workers) as pool:
        t = clock()
        pool.map(len, [()] * workers)
        T['pool start'] += clock() - t
        reads = [pool.apply_async(_timed_call, ('_read_annos', (root, split, b))) for b in batches[:2]]
        pending = []
        for k, idx in enumerate(batches):
            t = clock()
            an = torch.from_numpy(take(reads[k], 'worker seconds: annotation reads')).to(dev)
            T['wait for annotations'] += clock() - t
            if k + 2 < len(batches):
                reads.append(pool.apply_async(_timed_call, ('_read_annos', (root, split, batches[k + 2]))))
            t = clock()
            gt = DS.gt_batch(mano, an)
            verts = torch.cat((gt[1], gt[3]), dim=1).contiguous()
            m, d = V.render_frames(verts, faces, gt[8], colors, DS.IMG_SIZE, workspace=ws)
            nb = len(idx)
            if gpu_encode:
                enc(m, recs[:nb], nb)
                enc(d, recs[bs:bs + nb], nb)
            torch.cuda.synchronize()
            T['GT MANO + render (+ GPU encode)'] += clock() - t
            t = clock()
            if gpu_encode:
                host = recs.cpu().numpy()
                m, d = host[:nb], host[bs:bs + nb]
            else:
                m, d = m.cpu().numpy(), d.cpu().numpy()
            T['device-to-host'] += clock() - t
            t = clock()
            while len(pending) > 2 * workers:
                take(pending.pop(0), 'worker seconds: encode + write')
            T['wait for a free slot (workers behind)'] += clock() - t
            t = clock()
            for j in range(0, len(idx), chunk):
                pending.append(pool.apply_async(_timed_call, (write, (root, split, idx[j:j + chunk], m[j:j + chunk], d[j:j + chunk]))))
            T['submit to the pool (pickling)'] += clock() - t
            stamps.append(clock())
        t = clock()
        for p in pending:
            take(p, 'worker seconds: encode + write')
        T['drain at the end'] += clock() - t
    half = len(stamps) // 2
    T['images/s over the second half of the batches'] = (len(stamps) - 1 - half) * bs / (stamps[-1] - stamps[half]) if len(stamps) - 1 > half else float('nan')
    return n, clock() - t_all, T


def app(opt):
    import torch
    from fake_split import write_split
    from dir_amd import synth
    from dir_amd.apps import dataset as DS
    from dir_amd.apps import jpeg as AJ
    from dir_amd.apps import render_split as RS
    from dir_amd.utils import vis_utils as V
    tmp = tempfile.mkdtemp(prefix='bench_jpeg_enc_')
    try:
        root = os.path.join(tmp, 'data')
        write_split(root, 8, split='train', seed=1)                        # eight annotations, replicated: the tool reads anno/ only
        for i in range(8, opt.images):
            shutil.copy(os.path.join(root, 'train', 'anno', '%d.pkl' % (i % 8)), os.path.join(root, 'train', 'anno', '%d.pkl' % i))
        with open(os.path.join(ROOT, 'tests', 'golden', 'manifest_dir.json')) as fh:
            shapes = {k: tuple(v) for k, v in json.load(fh).items()}
        state = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in synth.synth_state_dict(shapes, 1234).items()}
        ckpt, dense = os.path.join(tmp, 'ckpt.pt'), os.path.join(tmp, 'dense.pkl')
        torch.save(state, ckpt)
        table = np.random.default_rng(11).random((778, 3))
        with open(dense, 'wb') as fh:
            pickle.dump(table, fh)
        modes = [('default', ROOT, []), ('--gpu_encode', ROOT, ['--gpu_encode'])]
        if opt.parent:
            modes.append(('parent commit, default', os.path.abspath(opt.parent), []))
        rate = {m[0]: [] for m in modes}
        wall = {m[0]: [] for m in modes}
        for _ in range(opt.runs):
            for name, tree, flags in modes:
                for kind in ('mask', 'dense'):
                    shutil.rmtree(os.path.join(root, 'train', kind), ignore_errors=True)
                r, w = _child(tree, root, ckpt, dense, flags)
                rate[name].append(r)
                wall[name].append(w)
        print('app: render_split of %d images (mask + dense each), bs 256, %d workers, %d runs per mode, alternating, each a child process' %
              (opt.images, RS.default_workers(), opt.runs))
        for name, _, _ in modes:
            print('  %-26s images/s inside the tool: %s ; wall seconds of the process: %s' % (name, spread(rate[name]), spread(wall[name])))

        # ---- where the time goes inside the running tool: its loop, clocked
        for name, flag in (('default', False), ('--gpu_encode', True)):
            for kind in ('mask', 'dense'):
                shutil.rmtree(os.path.join(root, 'train', kind), ignore_errors=True)
                os.makedirs(os.path.join(root, 'train', kind))
            n_img, wall_s, T = profiled_run(root, state, table, flag)
            print('inside the loop, %s: %d images in %.2f s (%.0f images/s with the clocks in); seconds of the main process per step, then of the workers (summed over %d workers):'
                  % (name, n_img, wall_s, n_img / wall_s, RS.default_workers()))
            for k, v in T.items():
                print('  %-48s %8.3f' % (k, v))

        # ---- the phases of one batch of 256, each alone in this process
        bs, dev = 256, 'cuda'
        mano = DS.gt_layers_from_checkpoint(state, dev)
        faces = torch.from_numpy(V.faces_from_layers(mano)).to(dev)
        colors = torch.from_numpy(V.load_dense_colors(table)).to(dev)
        from dir_amd import _capi
        ws = torch.empty(int(_capi.lib().dir_render_workspace_bytes(bs)), dtype=torch.uint8, device=dev)
        idx = list(range(bs))
        ph = {}

        def rec(name, fn, n=5):
            out = None
            ts = []
            for _ in range(n):
                t0 = time.perf_counter()
                out = fn()
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
            ph[name] = ts
            return out
        an = rec('annotation reads, one process (the tool: pool workers, two batches ahead)', lambda: RS._read_annos(root, 'train', idx))
        and_ = torch.from_numpy(an).to(dev)

        def render():
            gt = DS.gt_batch(mano, and_)
            return V.render_frames(torch.cat((gt[1], gt[3]), dim=1).contiguous(), faces, gt[8], colors, DS.IMG_SIZE, workspace=ws)
        render()
        m, d = rec('GT MANO + render (GPU)', render)
        enc = AJ.RecordEncoder(2 * bs, 256, 95)
        recs = torch.empty(2 * bs, enc.record_bytes, dtype=torch.uint8, device=dev)
        enc(m, recs[:bs]); enc(d, recs[bs:])
        rec('GPU encode of mask + dense (--gpu_encode)', lambda: (enc(m, recs[:bs]), enc(d, recs[bs:])))
        mh, dh = rec('device-to-host, frames (default)', lambda: (m.cpu().numpy(), d.cpu().numpy()))
        rh = rec('device-to-host, records (--gpu_encode)', lambda: recs.cpu().numpy())
        chunk = 16
        rec('pickle round trip of the batch in chunks of 16 (proxy of the pool transfer; same bytes in both modes)',
            lambda: [pickle.loads(pickle.dumps((root, 'train', idx[j:j + chunk], mh[j:j + chunk], dh[j:j + chunk]))) for j in range(0, bs, chunk)])
        out = os.path.join(tmp, 'w')
        for kind in ('mask', 'dense'):
            os.makedirs(os.path.join(out, 'train', kind), exist_ok=True)
        rec('Pillow encode + write, one process (default; the tool: %d workers)' % RS.default_workers(), lambda: RS._write(out, 'train', idx, mh, dh), 3)
        rec('Huffman encode + write, one process (--gpu_encode; the tool: %d workers)' % RS.default_workers(),
            lambda: RS._write_records(out, 'train', idx, rh[:bs], rh[bs:]), 3)
        files = [open(os.path.join(out, 'train', k, '%d.jpg' % i), 'rb').read() for k in ('mask', 'dense') for i in idx]

        def write_only():
            for j, b in enumerate(files):
                with open(os.path.join(out, 'w%d.jpg' % j), 'wb') as f:
                    f.write(b)
        rec('file writes alone (the %d files of the batch, mean %.0f bytes), one process' % (len(files), np.mean([len(b) for b in files])), write_only)
        import multiprocessing as mp

        def pool_start():
            with mp.get_context('spawn').Pool(RS.default_workers()) as pool:
                pool.map(len, [()] * RS.default_workers())
        rec('start of the spawned pool of %d workers until each has answered once (once per run of the tool, inside its clock)' % RS.default_workers(), pool_start, 2)
        print('phases of one batch of 256 images (512 frames), each alone in one process, ms per batch:')
        for k, v in ph.items():
            print('  %-100s %s' % (k, spread(v)))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('mode', choices=['kernels', 'host', 'app'])
    ap.add_argument('--rounds', type=int, default=None)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--frames', type=int, default=64)
    ap.add_argument('--images', type=int, default=1024)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--parent', type=str, default=None)
    opt = ap.parse_args()
    if opt.rounds is None:
        opt.rounds = 20 if opt.mode == 'kernels' else 5
    {'kernels': kernels, 'host': host, 'app': app}[opt.mode](opt)


if __name__ == '__main__':
    main()
