"""GPU: dir_jpeg_encode_records (csrc/jpeg_enc.hip) -- everything of cv.imwrite (dataset/prepare_data.py:174-214) before the Huffman coder
-- equals the numpy restatement (tests/helpers/jpeg_enc_ref.py, pinned to Pillow's libjpeg-turbo by tests/test_jpeg_enc_ref.py) byte for
byte: records of the committed and of generated frames, any slot of any batch, bytes beyond a record untouched, reruns and a graph replay;
the files written from its records are Pillow's files; the device round trip gives Pillow's decoded pixels; bad arguments fail before any
launch; render_split --gpu_encode writes the default path's files; TrainBatches(jpeg_round_trip=True) equals the file path."""
import ctypes as C
import os
import pickle
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, 'tests', 'helpers'))
import jpeg_enc_ref as R  # noqa: E402

from dir_amd import _capi  # noqa: E402
from dir_amd.apps import jpeg as AJ  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(ROOT, 'tests', 'golden', 'g26_jpeg_enc.npz')
SIZES = ((16, 16), (16, 32), (32, 16), (48, 80), (256, 256))
QUALITIES = (1, 50, 95, 100)


@pytest.fixture(scope='module')
def gold():
    g = np.load(GOLD)
    names = sorted(k[:-6] for k in g.files if k.endswith('.frame'))
    return {n: dict(frame=g[n + '.frame'], q=int(g[n + '.q']), jpg=g[n + '.jpg'].tobytes(), pix=g[n + '.pix']) for n in names}


def generated(h, w, seed=0):
    """noise with saturated patches and a flat region: every coefficient range, clipped chroma, zero blocks"""
    rng = np.random.RandomState(1000 * h + w + seed)
    a = np.clip(rng.normal(128, 80, (h, w, 3)), 0, 255).astype(np.uint8)
    a[: h // 4, : w // 2] = rng.randint(0, 2, (h // 4, w // 2, 3)) * 255
    a[h // 2:, w // 2:] = rng.randint(0, 256, 3)
    return a


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def encode(frames, quality, order='bgr', stride=None, fill=None):
    """frames uint8 [B,H,W,3] numpy -> records uint8 [B, stride] numpy"""
    B, H, W = frames.shape[:3]
    enc = AJ.RecordEncoder(B, (H, W), quality, order)
    stride = enc.record_bytes if stride is None else stride
    recs = torch.zeros(B, stride, dtype=torch.uint8, device='cuda') if fill is None else torch.full((B, stride), fill, dtype=torch.uint8, device='cuda')
    enc(dev(frames), recs)
    torch.cuda.synchronize()
    return recs.cpu().numpy()


def test_records_of_the_golden_frames_equal_the_restatement_and_pillow(gold):
    for n, c in gold.items():
        want = R.encode_record(c['frame'], c['q'])
        got = encode(c['frame'][None], c['q'])[0]
        assert got.size == want.size and np.array_equal(got[:512], want[:512]), n
        bad = np.flatnonzero(got[512:].view(np.int16) != want[512:].view(np.int16))
        assert bad.size == 0, (n, bad.size, bad[:8].tolist())
        assert AJ.record_to_bytes(got) == c['jpg'], n                     # GPU record -> host Huffman coder = the bytes Pillow wrote


@pytest.mark.parametrize('size', SIZES, ids=lambda s: '%dx%d' % s)
def test_records_of_generated_frames_equal_the_restatement(size):
    h, w = size
    f = generated(h, w)
    for q in QUALITIES:
        for order in ('bgr', 'rgb'):
            want = R.encode_record(f, q, order)
            got = encode(f[None], q, order)[0]
            assert np.array_equal(got[:512], want[:512]), (q, order)
            bad = np.flatnonzero(got[512:].view(np.int16) != want[512:].view(np.int16))
            assert bad.size == 0, (q, order, bad.size, bad[:8].tolist())


def test_any_slot_of_any_batch_gives_the_same_bytes():
    for h, w in ((48, 80), (256, 256)):
        f = generated(h, w, 1)
        alone = encode(f[None], 95)[0]
        assert np.array_equal(alone, R.encode_record(f, 95))
        five = np.stack([generated(h, w, 10 + i) for i in range(5)])
        five[3] = f
        r5 = encode(five, 95)
        assert np.array_equal(r5[3], alone)
        assert np.array_equal(r5[4], R.encode_record(five[4], 95))
        many = np.stack([generated(h, w, 20 + (i % 3)) for i in range(37)])
        many[29] = f
        r37 = encode(many, 95)
        assert np.array_equal(r37[29], alone)
        assert np.array_equal(r37[0], r37[3]) and np.array_equal(r37[36], r37[0]) and not np.array_equal(r37[0], r37[1])


def test_bytes_beyond_a_record_are_not_touched():
    f = np.stack([generated(48, 80, i) for i in range(3)])
    need = 512 + 48 * 80 * 3
    stride = need + 16 * 9
    got = encode(f, 50, stride=stride, fill=0xA5)
    for i in range(3):
        assert np.array_equal(got[i, :need], R.encode_record(f[i], 50)), i
        assert (got[i, need:] == 0xA5).all(), i
    # a partial batch: the records after the first n are not touched either
    enc = AJ.RecordEncoder(3, (48, 80), 50)
    recs = torch.full((3, stride), 0xA5, dtype=torch.uint8, device='cuda')
    enc(dev(f), recs, 2)
    torch.cuda.synchronize()
    assert np.array_equal(recs[:2].cpu().numpy(), got[:2]) and bool((recs[2] == 0xA5).all())


def test_reruns_and_a_graph_replay_give_identical_bytes():
    f = dev(np.stack([generated(256, 256, i) for i in range(4)]))
    enc = AJ.RecordEncoder(4, 256, 95)
    a = enc(f, torch.zeros(4, enc.record_bytes, dtype=torch.uint8, device='cuda'))
    b = enc(f, torch.zeros(4, enc.record_bytes, dtype=torch.uint8, device='cuda'))
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    out = torch.zeros(4, enc.record_bytes, dtype=torch.uint8, device='cuda')
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        enc(f, out)                                                       # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        enc(f, out)
    for _ in range(2):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, a)


def test_round_trip_equals_pillows_decode_of_pillows_file(gold):
    for n, c in gold.items():
        got = AJ.jpeg_round_trip(dev(c['frame'][None]), quality=c['q'])
        torch.cuda.synchronize()
        assert np.array_equal(got[0].cpu().numpy(), c['pix']), n
    # a batch, through the per-instance buffers, and the RGB order
    c = gold['rendered_256_q95']
    rt = AJ.RoundTrip(3, 256, 95, 'bgr')
    out = rt(dev(np.stack([c['frame']] * 3)))
    assert all(np.array_equal(out[i].cpu().numpy(), c['pix']) for i in range(3))
    rgb = AJ.RoundTrip(1, 256, 95, 'rgb')(dev(c['frame'][None, ..., ::-1]))
    assert np.array_equal(rgb[0].cpu().numpy(), c['pix'][..., ::-1])


def test_bad_arguments_fail_with_a_message_and_no_launch():
    L = _capi.lib()
    P = _capi.ptr
    luma, chroma = AJ.quality_tables(95)
    guard = torch.full((2, 512 + 32 * 32 * 3 + 64), 0xA5, dtype=torch.uint8, device='cuda')

    def call(frames, B, H, W, order, lq, cq, recs, stride):
        rc = L.dir_jpeg_encode_records(P(frames), B, H, W, order, lq.ctypes.data if lq is not None else None, cq.ctypes.data if cq is not None else None,
                                       P(recs), stride, _capi.stream_ptr())
        return rc, L.dir_last_error().decode()
    f = torch.zeros(2, 32, 32, 3, dtype=torch.uint8, device='cuda')
    stride = guard.shape[1]
    assert call(f, 2, 32, 32, 0, luma, chroma, guard, stride)[0] == 0
    torch.cuda.synchronize()
    good = guard.clone()
    guard.fill_(0xA5)
    zero = luma.copy()
    zero[17] = 0
    big = chroma.copy()
    big[3] = 256
    for args, word in (((f, 2, 24, 32, 0, luma, chroma, guard, stride), 'multiples of 16'),
                       ((f, 2, 32, 24, 0, luma, chroma, guard, stride), 'multiples of 16'),
                       ((f, 2, 0, 32, 0, luma, chroma, guard, stride), 'multiples of 16'),
                       ((f, 2, 4112, 32, 0, luma, chroma, guard, stride), '4096'),
                       ((f, 2, 32, 32, 2, luma, chroma, guard, stride), 'channel_order'),
                       ((f, 2, 32, 32, 0, zero, chroma, guard, stride), 'quantisation entry'),
                       ((f, 2, 32, 32, 0, luma, big, guard, stride), 'quantisation entry'),
                       ((f, 2, 32, 32, 0, luma, chroma, guard, 512 + 32 * 32 * 3 - 16), 'record_stride'),
                       ((f, 2, 32, 32, 0, luma, chroma, guard, 512 + 32 * 32 * 3 + 8), 'record_stride'),
                       ((f, 2, 32, 32, 0, None, chroma, guard, stride), 'bad arguments'),
                       ((None, 2, 32, 32, 0, luma, chroma, guard, stride), 'bad arguments'),
                       ((f, -1, 32, 32, 0, luma, chroma, guard, stride), 'bad arguments')):
        rc, msg = call(*args)
        assert rc == -1 and word in msg, (rc, msg, word)
    torch.cuda.synchronize()
    assert bool((guard == 0xA5).all())                                    # nothing was launched
    assert not torch.equal(good, guard)
    with pytest.raises(ValueError):
        AJ.RecordEncoder(1, 32, quality=0)
    with pytest.raises(ValueError):
        AJ.RecordEncoder(1, 32, quality=101)
    with pytest.raises(_capi.DirHipError, match='multiples of 16'):
        AJ.RecordEncoder(1, (24, 32))(torch.zeros(1, 24, 32, 3, dtype=torch.uint8, device='cuda'), torch.zeros(1, 4096, dtype=torch.uint8, device='cuda'))
    assert call(f, 0, 32, 32, 0, luma, chroma, guard, stride)[0] == 0     # an empty batch is not an error


# --------------------------------------------------------------------------------------------------------------------- the apps
@pytest.fixture(scope='module')
def state():
    import json
    from dir_amd import synth
    with open(os.path.join(ROOT, 'tests', 'golden', 'manifest_dir.json')) as fh:
        shapes = {k: tuple(v) for k, v in json.load(fh).items()}
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in synth.synth_state_dict(shapes, 1234).items()}


@pytest.fixture(scope='module')
def rendered_split(tmp_path_factory, state):
    """the fake split, rendered twice by the command-line tool: <a> by the default path, <b> with --gpu_encode"""
    from fake_split import write_split
    tmp = tmp_path_factory.mktemp('jpeg_enc_split')
    n = 5
    ckpt, dense = str(tmp / 'ckpt.pt'), str(tmp / 'dense.pkl')
    torch.save(state, ckpt)
    table = np.random.default_rng(11).random((778, 3))
    with open(dense, 'wb') as fh:
        pickle.dump(table, fh)
    roots = {}
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    for name, flags in (('a', []), ('b', ['--gpu_encode'])):
        roots[name] = str(tmp / name)
        write_split(roots[name], n, split='train', seed=2)
        r = subprocess.run([sys.executable, '-m', 'dir_amd.apps.render_split', '--save_path', roots[name], '--model', ckpt, '--dense_color', dense,
                            '--bs', '2', '--workers', '2'] + flags, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
    return roots, table, n


def test_render_split_gpu_encode_writes_the_default_paths_files(rendered_split):
    roots, table, n = rendered_split
    for kind in ('mask', 'dense'):
        names = sorted('%d.jpg' % i for i in range(n))
        assert sorted(os.listdir(os.path.join(roots['a'], 'train', kind))) == names == sorted(os.listdir(os.path.join(roots['b'], 'train', kind)))
        for f in names:
            with open(os.path.join(roots['a'], 'train', kind, f), 'rb') as fa, open(os.path.join(roots['b'], 'train', kind, f), 'rb') as fb:
                a, b = fa.read(), fb.read()
            assert len(a) > 600 and a == b, (kind, f, len(a), len(b))
    assert os.path.isdir(os.path.join(roots['b'], 'train', 'hms'))


def test_train_batches_with_the_round_trip_equal_the_file_path(rendered_split, state):
    from dir_amd.apps import dataset as DS
    from dir_amd.apps import trainset as T
    roots, table, n = rendered_split
    mano = DS.gt_layers_from_checkpoint(state)
    files = list(T.TrainBatches(roots['a'], mano, 'train', batch_size=2, workers=2, seed=4))
    trip = list(T.TrainBatches(roots['a'], mano, 'train', batch_size=2, workers=2, seed=4, dense_color=table, jpeg_round_trip=True))
    plain = list(T.TrainBatches(roots['a'], mano, 'train', batch_size=2, workers=2, seed=4, dense_color=table))
    torch.cuda.synchronize()
    assert len(files) == len(trip) == len(plain) == 2
    differs = False
    for fb, tb, pb in zip(files, trip, plain):
        for d in range(3):                                                # inputs, targets, meta_info
            assert sorted(fb[d]) == sorted(tb[d])
            for k in fb[d]:
                assert torch.equal(fb[d][k], tb[d][k]), k
        assert bool((tb[1]['seg'] > 0).any())
        differs = differs or not torch.equal(pb[1]['dense'], tb[1]['dense'])
    assert differs                                                        # the round trip is not a no-op on these frames
    # without the flag: today's frames, rendered and handed straight to augment_batch (tests/test_gpu_render.py pins those to the rasteriser's
    # restatement); they differ from the file path's only in mask_rgb / seg / dense
    import inspect
    assert inspect.signature(T.TrainBatches.__init__).parameters['jpeg_round_trip'].default is False
    for fb, pb in zip(files, plain):
        assert torch.equal(fb[0]['img'], pb[0]['img']) and torch.equal(fb[1]['mesh_3d_left'], pb[1]['mesh_3d_left'])
    with pytest.raises(ValueError):
        T.TrainBatches(roots['a'], mano, 'train', batch_size=2, workers=2, jpeg_round_trip=True)
