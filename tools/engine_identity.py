"""What one eager DirEngine.forward launches and computes, as text that two trees can be compared by: per configuration the sequence of
(entry point, kernels) of the profile records (_capi.PROFILE) and a sha256 of every tensor in outs_list.  B = 2, dir_amd/synth.py weights;
configurations: bf16, f16 storage, fp32, fp32 with arith='f16x3' after calibrate, and HRNet-W48 with one extra stage (bf16).

    python tools/engine_identity.py > identity.txt           # equal line for line between two trees that launch the same kernels
    python tools/engine_identity.py --time 50 > /dev/null    # also: host seconds of 50 eager forwards per configuration, on stderr

DIR_LIB_PATH selects the library, so two trees can be run on one build."""
import argparse
import hashlib
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from dir_amd import _capi, synth  # noqa: E402
from dir_amd.engine import DirEngine  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def digest(t):
    return hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--time', type=int, default=0, help='also time this many eager forwards per configuration (host clock, after 5 warm-up forwards)')
    args = ap.parse_args()
    torch.cuda.set_device(0)
    with open(os.path.join(ROOT, 'tests', 'golden', 'manifest_dir.json')) as f:
        shapes = {k: tuple(v) for k, v in json.load(f).items()}
    from dir_amd.models.dir import DIR
    net = DIR(21, 'x', 0, backbone='hrnet_w48', extra_stages=1)
    shapes_hr = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    del net
    img = torch.from_numpy(synth.synth_input('identity.img', (2, 3, 256, 256))).cuda()
    for tag, shp, dtype, arith in (('bf16', shapes, torch.bfloat16, None), ('f16', shapes, torch.float16, None), ('fp32', shapes, torch.float32, None),
                                   ('fp32_f16x3', shapes, torch.float32, 'f16x3'), ('hrnet_w48_x1_bf16', shapes_hr, torch.bfloat16, None)):
        sd = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in synth.synth_state_dict(shp, 1234).items()}
        eng = DirEngine(sd, dtype=dtype, arith=arith)
        eng.calibrate(img)                               # (returns at once unless arith is set)
        _capi.PROFILE = []
        try:
            outs = eng.forward(img)
            torch.cuda.synchronize()
            recs = _capi.PROFILE
        finally:
            _capi.PROFILE = None
        print('== %s: %d launches' % (tag, len(recs)))
        for i, r in enumerate(recs):
            print('%s %3d %s %s' % (tag, i, r['api'], r['kernels']))
        for i, o in enumerate(outs):
            for k in sorted(o):
                if o[k] is not None:
                    print('%s outs[%d][%s] %s %s' % (tag, i, k, tuple(o[k].shape), digest(o[k])))
        if args.time:
            for _ in range(5):
                eng.forward(img)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.time):
                eng.forward(img)
            host = time.perf_counter() - t0              # the host's share: the launches are queued, not waited for
            torch.cuda.synchronize()
            sys.stderr.write('TIME %s %d eager forwards: host %.4f s\n' % (tag, args.time, host))
        del eng, outs, recs
    sys.stdout.flush()


if __name__ == '__main__':
    main()
