"""GPU: apps.predict --separate -- after the forward every prediction's two hands go through the pair fit (dir_mano_fit_pair) with the pull to their own
parameters, the pull to their own offset and the capsule collision term -- and apps.fit_mano --pair.

The checkpoint is the synthetic one (random weights, synth.mano_buffers tables): its predictions are two random hands a few centimetres apart, and the
radii capsule_radii takes from random template vertices are centimetres wide, so every prediction overlaps.  Nothing here says anything about real hands."""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'helpers'))

from dir_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def state():
    with open(os.path.join(HERE, 'golden', 'manifest_dir.json')) as fh:
        shapes = {k: tuple(v) for k, v in json.load(fh).items()}
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in synth.synth_state_dict(shapes, 1234).items()}


@pytest.fixture(scope='module')
def eng(state):
    from dir_amd.engine import DirEngine
    return DirEngine(state, dtype=torch.float16, root_joint=0)


@pytest.fixture(scope='module')
def images(tmp_path_factory):
    from fake_split import write_split
    from PIL import Image

    from dir_amd.apps import dataset as DS
    d = tmp_path_factory.mktemp('separate')
    write_split(str(d / 'split'), 3, seed=8)
    ds = DS.InterHandSplit(str(d / 'split'))
    src = d / 'in'
    src.mkdir()
    for i in range(3):
        Image.fromarray(np.ascontiguousarray(ds.frame(i)[:, :, ::-1])).save(str(src / ('f%d.png' % i)), format='PNG')
    return d, src


def _files(d):
    return {n: open(os.path.join(d, n), 'rb').read() for n in sorted(os.listdir(d))}


def test_separate_with_weight_zero_keeps_the_hands_bit_for_bit(state, eng, images):
    """--separate --separate_weight 0: left / right / offset of every record equal the unflagged run's, and the unflagged command writes the same bytes
    before and after a flagged run in the same session"""
    from dir_amd.apps import predict as P
    d, src = images
    ck = str(d / 'DIR.pth')
    torch.save({'net': state}, ck)
    paths = [[str(src / ('f%d.png' % i)) for i in range(3)]]
    P.run(eng, paths, str(d / 'A'), bs=2, workers=2)
    before = _files(str(d / 'A'))
    assert P.main(['--model', ck, '--input', str(src), '--out', str(d / 'Z'), '--bs', '2', '--workers', '2', '--separate', '--separate_weight', '0']) == 3
    P.run(eng, paths, str(d / 'B'), bs=2, workers=2)
    assert _files(str(d / 'B')) == before
    flagged = _files(str(d / 'Z'))
    for n in sorted(before):
        r, p = json.loads(flagged[n]), json.loads(before[n])
        assert r['left'] == p['left'] and r['right'] == p['right'] and r['offset'] == p['offset'] and r['matrix'] == p['matrix']
        assert r['separated'] is False and r['collision']['after'] == r['collision']['before']
        assert r['unseparated']['left'] == p['left'] and r['unseparated']['right'] == p['right'] and r['unseparated']['offset'] == p['offset']
    with pytest.raises(SystemExit):
        P.main(['--model', ck, '--input', str(src), '--out', str(d / 'X'), '--separate_weight', '3'])


def test_separate_with_a_weight_reduces_the_overlap(state, eng, images):
    """--separate with its default weight: the records carry separated / collision / unseparated, "unseparated" is the unflagged run, and the largest
    capsule overlap after the fit is no larger than before on every record (and smaller on the separated ones)"""
    from dir_amd.apps import predict as P
    d, src = images
    ck = str(d / 'DIR2.pth')
    torch.save({'net': state}, ck)
    paths = [[str(src / ('f%d.png' % i)) for i in range(3)]]
    P.run(eng, paths, str(d / 'P'), bs=2, workers=2)
    plain = _files(str(d / 'P'))
    assert P.main(['--model', ck, '--input', str(src), '--out', str(d / 'S'), '--bs', '2', '--workers', '2', '--separate', '--separate_iters', '30']) == 3
    flagged = _files(str(d / 'S'))
    moved = 0
    for n in sorted(plain):
        r, p = json.loads(flagged[n]), json.loads(plain[n])
        c = r['collision']
        print(n, 'separated', r['separated'], 'max overlap mm %.2f -> %.2f' % (c['before']['max_overlap'] * 1e3, c['after']['max_overlap'] * 1e3))
        assert set(c) == {'before', 'after'} and set(c['before']) == {'mean_sq_overlap', 'max_overlap'}
        assert c['after']['max_overlap'] <= c['before']['max_overlap']
        assert r['unseparated']['left'] == p['left'] and r['unseparated']['right'] == p['right'] and r['unseparated']['offset'] == p['offset']
        if r['separated']:
            moved += 1
            assert c['after']['max_overlap'] < c['before']['max_overlap'] and r['offset'] != p['offset']
        else:
            assert r['left'] == p['left'] and r['right'] == p['right'] and r['offset'] == p['offset']
    assert moved >= 1


def test_fit_mano_command_with_and_without_pair(state, tmp_path, capsys):
    """apps.fit_mano --pair on 3-D joints of two overlapping hands: O.npz gains offset, collision and pair_status, the overlap falls, and the unflagged
    command writes the same file before and after"""
    import mano_fit_ref as R
    import mano_pair_fit_ref as PR

    from dir_amd.apps import fit_mano as A
    tg = {}
    for side, seed in (('left', 0), ('right', 1)):
        p = R.truth(4, side, seed)[1:]                            # (centred at the wrist, pair 0 does not overlap)
        t = R.targets_of(p, side, 0)
        tg['joints_' + side], tg['init_' + side] = t['joints'], p
    tg['offset'] = np.asarray(PR.OFFSETS[1:4], np.float32)
    np.savez(str(tmp_path / 'T.npz'), **tg)
    np.savez(str(tmp_path / 'R.npz'), radii_left=PR.radii_np(), radii_right=PR.radii_np()[::-1].copy())
    ck = str(tmp_path / 'DIR.pth')
    torch.save({'net': state}, ck)
    common = ['--model', ck, '--targets', str(tmp_path / 'T.npz'), '--iters', '40', '--lr', '0.01', '--lr_betas', '0', '--w_init', '0.01']
    assert A.main(common + ['--out', str(tmp_path / 'A.npz')]) == 6
    assert A.main(common + ['--out', str(tmp_path / 'P.npz'), '--pair', '--radii', str(tmp_path / 'R.npz'), '--w_offset_init', '1', '--lr_offset', '0.003']) == 6
    assert 'largest capsule overlap' in capsys.readouterr().out
    assert A.main(common + ['--out', str(tmp_path / 'B.npz')]) == 6
    assert open(str(tmp_path / 'A.npz'), 'rb').read() == open(str(tmp_path / 'B.npz'), 'rb').read()
    a, p = np.load(str(tmp_path / 'A.npz')), np.load(str(tmp_path / 'P.npz'))
    assert sorted(p.files) == sorted(a.files + ['offset', 'collision', 'pair_status'])
    print('max overlap mm', (p['collision'][:, 1] * 1e3).tolist(), '->', (p['collision'][:, 3] * 1e3).tolist())
    assert p['pair_status'].tolist() == [0] * 3 and p['offset'].shape == (3, 3) and (p['collision'][:, 1] > 5e-3).all()
    assert (p['collision'][:, 3] < 0.5 * p['collision'][:, 1]).all()
    with pytest.raises(SystemExit):
        A.main(common + ['--out', str(tmp_path / 'X.npz'), '--pair', '--center', '-1'])
