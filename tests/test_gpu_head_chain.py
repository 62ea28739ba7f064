"""The decoder's last four convolutions as two chained launches (dir_amd/engine/decoder.py::ConvChainOp over conv_as.hip's chained mode): conv_final.0 ->
conv_final.3 (models/dir.py:474-476) and the merged seg | dense 3x3 -> their 1x1s (models/dir.py:425-433).  With DIR_HEAD_CHAIN off and on the
whole forward -- every output, every tap -- is torch.equal, a captured graph replays the same bits, and the kernel table keeps ONE ROW PER LAYER:
the same 52 rows in the same order either way, so the shipped table loads unchanged."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
from dir_amd import _capi, synth
from dir_amd import engine as E

pytestmark = pytest.mark.gpu
SEED = 1234
GOLDEN = os.path.join(ROOT, 'tests', 'golden')


@pytest.fixture(scope='module')
def dir_state():
    with open(os.path.join(GOLDEN, 'manifest_dir.json')) as f:
        shapes = {k: tuple(v) for k, v in json.load(f).items()}
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in synth.synth_state_dict(shapes, SEED).items()}


@pytest.fixture(scope='module')
def shipped():
    with open(os.path.join(ROOT, 'dir_amd', 'tuning', 'gfx950_bf16_b64_throughput.json')) as f:
        return json.load(f)['table']


class chain(object):
    """with chain(on): ... -- the class switch, restored afterwards"""
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.saved, E.ConvChainOp.head_chain = E.ConvChainOp.head_chain, self.on

    def __exit__(self, *a):
        E.ConvChainOp.head_chain = self.saved


def _run(eng, img):
    taps = {}
    outs = eng.forward(img, taps=taps)
    torch.cuda.synchronize()
    return [{k: v.clone() for k, v in o.items() if torch.is_tensor(v)} for o in outs], {k: v.clone() for k, v in taps.items()}


@pytest.mark.parametrize('dt', [torch.bfloat16, torch.float16])
def test_forward_taps_and_graph_replay_are_bit_identical(dir_state, dt):
    eng = E.DirEngine(dir_state, dtype=dt)
    assert eng.final_chain.w is not None and eng.heads_chain.w is not None
    img = torch.randn(3, 3, 256, 256, device='cuda', generator=torch.Generator(device='cuda').manual_seed(8))
    with chain(False):
        outs0, taps0 = _run(eng, img)
    with chain(True):
        outs1, taps1 = _run(eng, img)
        n = 0
        for o0, o1 in zip(outs0, outs1):
            assert o0.keys() == o1.keys()
            for k, v in o0.items():
                assert torch.equal(v, o1[k]), k
                n += 1
        assert n > 20 and 'seg' in outs0[-1] and 'dense' in outs0[-1] and outs0[-1]['seg'].dtype == torch.float32
        assert taps0.keys() == taps1.keys() and 'final' in taps0
        for k, v in taps0.items():
            assert torch.equal(v, taps1[k]), k
        # captured-graph replay of the chained forward = eager
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            eng.forward(img)
            s.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                outs_g = eng.forward(img)
            g.replay()
        torch.cuda.synchronize()
        for o0, og in zip(outs0, outs_g):
            for k, v in o0.items():
                assert torch.equal(v, og[k]), 'graph: ' + k


def _conv_records(eng, img):
    saved = _capi.PROFILE
    _capi.PROFILE = []
    try:
        eng.forward(img)
        torch.cuda.synchronize()
        return [r for r in _capi.PROFILE if r.get('family') == 'conv']
    finally:
        _capi.PROFILE = saved


def test_table_rows_are_layers_and_the_launch_log_has_no_standalone_1x1(dir_state, shipped):
    eng = E.DirEngine(dir_state, dtype=torch.bfloat16)
    img = torch.randn(2, 3, 256, 256, device='cuda', generator=torch.Generator(device='cuda').manual_seed(6))
    assert len(shipped) == 52
    covered = (eng.final3, eng.heads3)
    for on in (False, True):
        with chain(on):
            eng.import_tuning(img, shipped)                         # raises ValueError when rows and layers differ
            assert eng.export_tuning(2) == [list(r) for r in shipped], on
            assert eng._tuned_order[2][-4:] == [eng.final0, eng.final3, eng.heads0, eng.heads3]
            recs = _conv_records(eng, img)
            # every conv-family record is a real launch with work announced (what the benchmark's roofline reads)
            assert all(r['kernels'] and r['bytes'] > 0 and r['flops'] > 0 and r['e0'].elapsed_time(r['e1']) > 0 for r in recs)
            alone = [r for r in recs if r.get('op') in covered]
            chained = [r for r in recs if r['api'] == 'dir_conv2d_as_chain_forward']
            if on:
                assert not alone and len(chained) == 2
                assert [r['op'] for r in chained] == [eng.final0, eng.heads0] and [r['covers'] for r in chained] == [(eng.final3,), (eng.heads3,)]
                assert all(r['kernels'].count('conv_as_kernel') == 1 and ',' not in r['kernels'] for r in chained)
                assert len(recs) == n_off - 2
                for r in chained:                                   # flops and bytes of both layers
                    c3, c1 = r['op'], r['covers'][0]
                    m = 2 * 32 * 32
                    assert r['flops'] == 2.0 * m * (256 * 9 * 256 + c1.cout * 256)
                    assert r['bytes'] == m * 256 * 2 + (c3.w.numel() + c1.w.numel()) * 2 + m * c1.cout * (4 if c1 is eng.heads3 else 2)
            else:
                assert len(alone) == 2 and not chained
                n_off = len(recs)
    with chain(True):
        eng.autotune(img, reps=1)
        table = eng.export_tuning(2)
    assert [r[:5] for r in table] == [list(r[:5]) for r in shipped]      # still 52 rows, in engine order
    with chain(False):                                                   # and a table made with the chain on serves the four launches
        eng.import_tuning(img, table)
        assert eng.export_tuning(2) == table


def test_an_fp32_engine_has_no_chained_pair(dir_state):
    eng = E.DirEngine(dir_state, dtype=torch.float32)
    assert eng.final_chain.w is None and eng.heads_chain.w is None
