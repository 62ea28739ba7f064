"""Per-launch times of layer3's identity blocks 1-5 inside whole eager forwards (profiles/l3_chain_per_block.txt): B = 64, both 16-bit storage
kinds, the time-tuned and the shipped throughput table, 7 forwards after a warm-up one.  Run it from the root of the tree to be measured (the
parent commit's checkout for BEFORE, this one for AFTER); the lines are appended to OUTFILE.
usage: python tools/l3_chain_per_block.py LABEL OUTFILE"""
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.getcwd())
from dir_amd import engine as E, synth  # noqa: E402

label, outfile = sys.argv[1], sys.argv[2]
with open(os.path.join('tests', 'golden', 'manifest_dir.json')) as f:
    shapes = {k: tuple(v) for k, v in json.load(f).items()}
sd = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in synth.synth_state_dict(shapes, 1234, cond=True).items()}
lines = []
for dt in (torch.float16, torch.bfloat16):
    eng = E.DirEngine(sd, dtype=dt)
    img = torch.randn(64, 3, 256, 256, device='cuda', generator=torch.Generator(device='cuda').manual_seed(1234))
    eng.forward(img)
    torch.cuda.synchronize()
    eng.autotune(img)
    for table in ('time-tuned', 'shipped'):
        if table == 'shipped':
            assert eng.load_tuning_table(img, 'gfx950_bf16_b64_throughput') is not None
        eng._profiled_forwards(img, 1)
        recs = eng._profiled_forwards(img, 7)
        ms = lambda r: r['e0'].elapsed_time(r['e1']) * 1e3      # noqa: E731
        total = sum(ms(r) for r in recs) / 7
        block_sums = []
        for bi, blk in enumerate(eng.bb.layers[2][1:], start=1):
            ops = [blk['c2']] + ([blk['tail']] if 'tail' in blk else [blk['c3']])
            parts, per_fwd = [], None
            for op in ops:
                ts = [ms(r) for r in recs if r['op'] is op]
                if not ts:
                    continue
                assert len(ts) == 7
                kern = [r['kernels'] for r in recs if r['op'] is op][0]
                kern = kern.split(',')[0]
                parts.append((kern, ts))
            per_fwd = [sum(p[1][i] for p in parts) for i in range(7)]
            med = statistics.median(per_fwd)
            block_sums.append(med)
            lines.append('%s %-8s %-10s layer3.%d  %s  sum: min %.1f us, median %.1f us, spread of the 7 forwards %.1f us' % (
                label, str(dt).split('.')[-1], table, bi,
                ' | '.join('%s min %.1f med %.1f' % (k, min(t), statistics.median(t)) for k, t in parts), min(per_fwd), med, max(per_fwd) - min(per_fwd)))
        lines.append('%s %-8s %-10s five blocks: median sum %.1f us; all conv-family launches of a forward: mean sum %.1f us' % (
            label, str(dt).split('.')[-1], table, sum(block_sums), total))
    del eng
with open(outfile, 'a') as f:
    f.write('\n'.join(lines) + '\n')
print('\n'.join(lines))
