"""GPU: dir_amd.apps.predict -- full frames -> GPU crops -> DirEngine.forward -> predictions in frame pixels, with synthetic weights.

  embedded tiles   256 x 256 frames placed at integer offsets in larger canvases, boxes that make the crop a pure translation: the crops
                   are the tiles, every tensor of stages 0-2 is bit-identical to DirEngine.forward on the tiles, joints_px = crop
                   pixels + offset
  command line     main() on a directory of PNGs of mixed sizes with a boxes.json that covers some of them: the files, the JSON fields,
                   the picture halves, the OBJ
  --track          two sequences of three frames in lockstep: the device chain equals the host chain bit for bit, a held box included"""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'helpers'))
import crop_ref as R  # noqa: E402
from fake_split import write_split  # noqa: E402

from dir_amd import synth  # noqa: E402
from dir_amd.apps import dataset as DS  # noqa: E402
from dir_amd.apps import predict as P  # noqa: E402
from dir_amd.utils import crop as CR  # noqa: E402
from dir_amd.utils import vis_utils as V  # noqa: E402

pytestmark = pytest.mark.gpu

CANVASES = [((300, 400), (70, 40)), ((512, 334), (0, 256)), ((281, 700), (444, 25)), ((256, 256), (0, 0))]       # (H, W), (ox, oy)
STAGE_KEYS = ('pd_joint_uv_left', 'pd_joint_uv_right', 'pd_mesh_xyz_left', 'pd_mesh_xyz_right', 'pd_joint_xyz_left', 'pd_joint_xyz_right',
              'pd_proj_left', 'pd_proj_right', 'pd_offset', 'pd_rel_joint')


@pytest.fixture(scope='module')
def state():
    with open(os.path.join(HERE, 'golden', 'manifest_dir.json')) as fh:
        shapes = {k: tuple(v) for k, v in json.load(fh).items()}
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in synth.synth_state_dict(shapes, 1234).items()}


@pytest.fixture(scope='module')
def eng(state):
    from dir_amd.engine import DirEngine
    return DirEngine(state, dtype=torch.float16)


@pytest.fixture(scope='module')
def tiles(tmp_path_factory):
    root = str(tmp_path_factory.mktemp('tiles'))
    write_split(root, 4, seed=5)
    ds = DS.InterHandSplit(root)
    return [np.ascontiguousarray(ds.frame(i)) for i in range(4)]


def embed(tiles, seed=0):
    """-> (canvases, boxes): every tile at its integer offset in a canvas of random bytes; the box spans the tile, so that at ratio 1
    mid = offset + 128, L = 128, s = 1: a pure translation by -offset"""
    rng = np.random.default_rng(seed)
    canvases, boxes = [], []
    for t, ((h, w), (ox, oy)) in zip(tiles, CANVASES):
        c = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
        c[oy:oy + 256, ox:ox + 256] = t
        canvases.append(c)
        boxes.append([ox, oy, ox + 256, oy + 256])
    return canvases, boxes


def same_bits(a, b):
    if a is None or b is None:
        return a is b
    a, b = a.contiguous(), b.contiguous()
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def test_embedded_tiles(eng, tiles):
    canvases, boxes = embed(tiles)
    tr = P.Tracker(eng, ratio=1.0, stage=2, track=False)
    crops, outs = tr.step(CR.FrameBatch(canvases), boxes)
    outs = [{k: None if v is None else v.clone() for k, v in o.items()} for o in outs[:3]]
    assert np.array_equal(tr.M.cpu().numpy(), [[1, 0, -ox, 0, 1, -oy] for _, (ox, oy) in CANVASES]) and tr.valid.cpu().tolist() == [1] * 4
    assert np.array_equal(crops.cpu().numpy(), np.stack(tiles))
    want = eng.forward(torch.from_numpy(np.stack(tiles)).cuda(), want_proj_feat=False)
    torch.cuda.synchronize()
    for s in range(3):
        assert sorted(outs[s]) == sorted(STAGE_KEYS)
        for k in STAGE_KEYS:
            assert same_bits(outs[s][k], want[s][k]), (s, k)
    recs = P.predict(eng, canvases, boxes, ratio=1.0, stage=2, bs=4, keep_crops=True)
    for j, (r, (_, (ox, oy))) in enumerate(zip(recs, CANVASES)):
        assert np.array_equal(r['crop'], tiles[j]) and r['valid'] and not r['tracked'] and r['box'] == [float(v) for v in boxes[j]]
        assert r['matrix'] == [[1.0, 0.0, -float(ox)], [0.0, 1.0, -float(oy)]] and (r['height'], r['width']) == CANVASES[j][0]
        for side in ('left', 'right'):
            uv = want[2]['pd_joint_uv_' + side][j].float().cpu().numpy().astype(np.float64)
            px = ((uv + 1) * 128 + np.float64([ox, oy])).astype(np.float32)             # crop pixels + offset, rounded once
            assert np.array_equal(np.float32(r[side]['joints_px']), px), (j, side)
            assert np.array_equal(np.float32(r[side]['joints_xyz']), want[2]['pd_joint_xyz_' + side][j].float().cpu().numpy())
    # bs = 3: two batches (3 + 1) give the same crops; the last image alone is still its tile
    recs3 = P.predict(eng, canvases, boxes, ratio=1.0, bs=3, keep_crops=True)
    assert all(np.array_equal(a['crop'], b['crop']) and a['matrix'] == b['matrix'] for a, b in zip(recs, recs3))


def save_png(path, bgr):
    from PIL import Image
    Image.fromarray(np.ascontiguousarray(bgr[:, :, ::-1])).save(path, format='PNG')


def test_predict_command(tmp_path, state, eng, tiles, capsys):
    """main() on PNGs of mixed sizes, two of four with a box; bs 3 -> batches of 3 + 1.  The JSON matrices are the restatement's, the
    picture's halves are the crop and overlay_predictions of the same batch byte for byte, the OBJ holds both hands"""
    from PIL import Image
    canvases, boxes = embed(tiles, seed=1)
    src, out = tmp_path / 'in', str(tmp_path / 'out')
    src.mkdir()
    names = ['f10.png', 'f2.png', 'f1.png', 'f3.png']                    # natural order: f1, f2, f3, f10
    for n, c in zip(names, canvases):
        save_png(str(src / n), c)
    order = [2, 1, 3, 0]
    given = {'f1.png': [60.5, 30, 340, 300], 'f10': boxes[0]}             # by name and by stem; f2 and f3 use the whole frame
    with open(tmp_path / 'boxes.json', 'w') as f:
        json.dump(given, f)
    ck = str(tmp_path / 'DIR.pth')
    torch.save({'net': state}, ck)
    n = P.main(['--model', ck, '--input', str(src), '--out', out, '--boxes', str(tmp_path / 'boxes.json'), '--bs', '3', '--workers', '2',
                '--pictures', '--obj'])
    lines = capsys.readouterr().out.strip().splitlines()
    assert n == 4 and lines[-1].startswith('4 images in ') and lines[-1].endswith('images/s')
    stems = ['f1', 'f2', 'f3', 'f10']
    assert sorted(os.listdir(out)) == sorted(s + e for s in stems for e in ('.json', '.png', '.obj'))
    mano = DS.gt_layers_from_checkpoint(state)
    r = V.mano_two_hands_shaded_renderer(right_faces=mano['right'].get_faces(), dense_color=np.zeros((778, 3)), img_size=256, device='cuda')
    used = [given['f1.png'], None, None, boxes[0]]
    for b0, b1 in ((0, 3), (3, 4)):
        fr = [canvases[order[j]] for j in range(b0, b1)]
        bx = [used[j] if used[j] is not None else [0, 0, f.shape[1] - 1, f.shape[0] - 1] for j, f in zip(range(b0, b1), fr)]
        M, valid = CR.crop_matrices_from_boxes(torch.tensor(bx, dtype=torch.float32).cuda(), 0.8, 256)
        crops = CR.crop_frames(CR.FrameBatch(fr), M, valid, 256)
        outs = eng.forward(crops, want_proj_feat=False)
        over = V.overlay_predictions(outs[2], crops, r).cpu().numpy()
        _, _, vl, vr = V.prediction_camera(outs[2])
        for j in range(b0, b1):
            with open(os.path.join(out, stems[j] + '.json')) as f:
                rec = json.load(f)
            assert sorted(rec) == sorted(['image', 'width', 'height', 'box', 'matrix', 'valid', 'tracked', 'left', 'right', 'offset'])
            assert rec['image'] == stems[j] + '.png' and (rec['height'], rec['width']) == fr[j - b0].shape[:2]
            assert rec['valid'] is True and rec['tracked'] is False and rec['box'] == [float(v) for v in bx[j - b0]]
            want_M, ok = R.matrix_from_box(bx[j - b0], 0.8, 256)
            assert ok == 1 and np.array_equal(np.float64(rec['matrix']).view(np.uint64), want_M.view(np.uint64))
            for side in ('left', 'right'):
                h = rec[side]
                assert np.shape(h['joints_px']) == (21, 2) and np.shape(h['joints_xyz']) == (21, 3) and np.shape(h['camera_px']['trans']) == (2,)
                px = CR.to_frame_pixels(outs[2]['pd_joint_uv_' + side].float(), M)[j - b0].cpu().numpy()
                assert np.array_equal(np.float32(h['joints_px']), px)
            assert len(rec['offset']) == 3
            with Image.open(os.path.join(out, stems[j] + '.png')) as im:
                pic = np.asarray(im.convert('RGB'))[:, :, ::-1]
            assert pic.shape == (256, 512, 3)
            assert np.array_equal(pic[:, :256], crops[j - b0].cpu().numpy()) and np.array_equal(pic[:, 256:], over[j - b0]), stems[j]
            with open(os.path.join(out, stems[j] + '.obj')) as f:
                rows = [l.split() for l in f if l[:2] in ('v ', 'f ')]
            v = np.float32([x[1:] for x in rows if x[0] == 'v'])
            fc = np.int64([x[1:] for x in rows if x[0] == 'f'])
            assert v.shape == (1556, 3) and fc.shape == (3076, 3) and fc.min() == 1 and fc.max() == 1556
            assert np.abs(v - torch.cat((vl, vr), 1)[j - b0].cpu().numpy()).max() < 1e-6
    # the image with the whole-frame box: the crop shows the whole frame, shrunk; its corners are border
    with open(os.path.join(out, 'f2.json')) as f:
        rec = json.load(f)
    assert rec['box'] == [0.0, 0.0, 333.0, 511.0] and rec['matrix'][0][0] == 128 / (511 / 2 / 0.8)


def test_track(tmp_path, state, eng, tiles, capsys):
    """Two sequences of three frames in lockstep, through predict(track=True) and through main(--track) on sub-directories.  Every frame's
    matrix and `tracked` flag equal the restatement applied on the host to the previous frame's read-back stage, bit for bit.

    With the synthetic weights the predicted cameras are not those of a trained network, so the first boxes are chosen to bring both
    branches about whatever it predicts: sequence 1 starts from a 6 px box (s = 34), and any prediction that fills less than half of its
    crop then asks for s > 64 and holds.  At least one of the four steps must hold; which ones do is printed."""
    rng = np.random.default_rng(9)
    seqs, first = [], []
    for q, ((h, w), (ox, oy)) in enumerate(CANVASES[:2]):
        frames = []
        for t in range(3):
            c = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
            c[oy:oy + 256, ox:ox + 256] = tiles[(q + t) % 4]
            frames.append(c)
        seqs.append(frames)
        # sequence 0 starts from the tile's hands-sized box (s = 0.74), sequence 1 from a 6 px box (s = 34): any prediction that fills less
        # than half of ITS crop then asks for s > 64, which no box gives: it holds
        first.append([ox + 20.0, oy + 20.0, ox + 236.0, oy + 236.0] if q == 0 else [ox + 125.0, oy + 125.0, ox + 131.0, oy + 131.0])
    recs = P.predict(eng, seqs, first, ratio=0.8, stage=2, track=True, keep_stage=True, keep_crops=True)
    assert [len(r) for r in recs] == [3, 3]
    flags = []
    for q in range(2):
        M0, ok0 = R.matrix_from_box(first[q], 0.8, 256)
        assert ok0 == 1 and np.array_equal(np.float64(recs[q][0]['matrix']).view(np.uint64), M0.view(np.uint64))
        assert recs[q][0]['tracked'] is False and recs[q][0]['valid'] is True and recs[q][0]['box'] == first[q]
        for t in range(1, 3):
            prev, cur = recs[q][t - 1], recs[q][t]
            st = prev['stage']
            want, ok = R.matrix_from_meshes(st['pd_mesh_xyz_left'], st['pd_mesh_xyz_right'], st['pd_proj_left'], st['pd_proj_right'],
                                            np.float64(prev['matrix']), 0.8, 256)
            assert np.array_equal(np.float64(cur['matrix']).view(np.uint64), want.view(np.uint64)), (q, t)
            assert cur['tracked'] is bool(ok) and cur['valid'] is True and cur['box'] is None, (q, t)
            if not ok:
                assert cur['matrix'] == prev['matrix']
            flags.append(bool(ok))
            # the crop is the frame warped with the recorded matrix
            got = CR.crop_frames(CR.FrameBatch([seqs[q][t]]), torch.tensor(cur['matrix'], dtype=torch.float64).reshape(1, 6).cuda())
            assert np.array_equal(got[0].cpu().numpy(), cur['crop']), (q, t)
    print('tracked flags (sequence 0 frames 1, 2; sequence 1 frames 1, 2):', flags)
    assert False in flags                                                 # a held box is part of the case
    # the command on the same frames as files: the same matrices and flags
    src, out = tmp_path / 'video', str(tmp_path / 'out')
    for q, name in enumerate(('a', 'b')):
        (src / name).mkdir(parents=True)
        for t in range(3):
            save_png(str(src / name / ('%d.png' % t)), seqs[q][t])
    with open(tmp_path / 'boxes.json', 'w') as f:
        json.dump({}, f)
    ck = str(tmp_path / 'DIR.pth')
    torch.save({'net': state}, ck)
    whole = P.predict(eng, seqs, None, ratio=0.8, stage=2, track=True)
    assert P.main(['--model', ck, '--input', str(src), '--out', out, '--track', '--boxes', str(tmp_path / 'boxes.json')]) == 6
    assert capsys.readouterr().out.strip().splitlines()[-1].startswith('6 images in ')
    for q, name in enumerate(('a', 'b')):
        assert sorted(os.listdir(os.path.join(out, name))) == ['0.json', '1.json', '2.json']
        for t in range(3):
            with open(os.path.join(out, name, '%d.json' % t)) as f:
                rec = json.load(f)
            assert rec['matrix'] == whole[q][t]['matrix'] and rec['tracked'] == whole[q][t]['tracked'] and rec['image'] == '%d.png' % t
            assert rec['left']['joints_px'] == whole[q][t]['left']['joints_px']

