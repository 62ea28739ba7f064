"""Rate of the training input: TrainBatches over a synthetic train split (tests/helpers/fake_train_split.py's layout), images/s, and the
GPU time of the augmentation launches alone (HIP events around augment_batch on decoded frames).

  python tools/train_input_rate.py [--n 512] [--bs 32] [--workers 8] [--records 1] [--dense_color 0] [--out FILE]

--dense_color 1: mask / dense rendered on the GPU from the GT meshes (TrainBatches(dense_color=...)) instead of decoded from files."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, 'tests', 'helpers')]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=512)
    ap.add_argument('--bs', type=int, default=32)
    ap.add_argument('--workers', type=int, default=8)
    ap.add_argument('--records', type=int, default=1)
    ap.add_argument('--dense_color', type=int, default=0)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    from fake_train_split import write_train_split
    from dir_amd import synth
    from dir_amd.apps import dataset as DS
    from dir_amd.apps import trainset as T
    with open(os.path.join(REPO, 'tests', 'golden', 'manifest_dir.json')) as f:
        shapes = {k: tuple(v) for k, v in json.load(f).items()}
    sd = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in synth.synth_state_dict(shapes, 1234).items() if 'mano_layer' in k}
    mano = DS.gt_layers_from_checkpoint(sd)
    res = {}
    # the augmentation launches alone, B = bs, on frames already on the GPU
    B = a.bs
    fr = [torch.randint(0, 256, (B, 256, 256, 3), dtype=torch.uint8, device='cuda') for _ in range(3)]
    an = torch.zeros(B, DS.ANNO_FLOATS, device='cuda')
    an[:, 0:9] = torch.eye(3, device='cuda').reshape(9)
    an[:, 11] = 0.8
    an[:, 12:21] = torch.tensor([[1500., 0, 128], [0, 1500, 128], [0, 0, 1]], device='cuda').reshape(9)
    for h in range(2):
        an[:, 21 + 67 * h:30 + 67 * h] = torch.eye(3, device='cuda').reshape(9)
    gt = DS.gt_batch(mano, an)
    P = T.params_to_device(T.sample_params(np.random.default_rng(0), B), 'cuda')
    scratch = torch.empty(B, 256, 256, 3, dtype=torch.uint8, device='cuda')
    for _ in range(5):
        T.augment_batch(*fr, gt, P, seed=1, scratch=scratch)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps = 50
    e0.record()
    for _ in range(reps):
        T.augment_batch(*fr, gt, P, seed=1, scratch=scratch)
    e1.record()
    torch.cuda.synchronize()
    res['augment_batch_ms_per_batch'] = e0.elapsed_time(e1) / reps
    res['batch'] = B
    with tempfile.TemporaryDirectory() as d:
        t0 = time.perf_counter()
        write_train_split(d, a.n, seed=0)
        res['write_split_s'] = time.perf_counter() - t0
        table = np.random.default_rng(0).random((778, 3)) if a.dense_color else None
        tb = T.TrainBatches(d, mano, 'train', batch_size=a.bs, workers=a.workers, seed=0, records=bool(a.records), dense_color=table)
        for _ in tb:                                              # first epoch: spawn + warm-up
            pass
        torch.cuda.synchronize()
        k, t0, t_start = 0, None, time.perf_counter()
        for inputs, targets, meta in tb:
            if t0 is None:                                        # steady state: from the first batch of the epoch on
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                continue
            k += inputs['img'].shape[0]
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    res.update(images=k, seconds=dt, images_per_sec=k / dt, workers=a.workers, records=bool(a.records), dense_color=bool(a.dense_color),
               epoch_start_s=t0 - t_start, note='second epoch after its first batch (the decode processes of the epoch are up)')
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'a') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
