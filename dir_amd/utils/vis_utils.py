"""Two-hand mesh rendering of utils/vis_utils.py (mano_two_hands_renderer) on csrc/render.hip, for dataset/prepare_data.py:174-214
(render_data: the mask/ and dense/ frames of the prepared split) and the training input.

  rasterize         verts [B,1556,3] (camera frame) + faces + K -> pix_to_face / zbuf / bary / colour images (dir_render_two_hands)
  render_frames     -> the mask and dense uint8 frames cv.imwrite receives in render_data (array channel order)
  mano_two_hands_renderer
                    the reference class for the `cameras=` path: render_mask, render_densepose -> (img, alpha), render_depth -> zbuf
                    [B,S,S,1]; values as the reference returns them (texel / 255, background 1 / 255)

The rasteriser restates pytorch3d's rasterize_meshes (blur_radius 0, faces_per_pixel 1, perspective-correct, no culling) and the
HardPhongShader + AmbientLights texel; the rules are in csrc/render.hip.  Parity: bit-exact with a numpy restatement of those rules
(tests/helpers/raster_ref.py), unpinned against pytorch3d, which is not installed where this was written.  Orthographic cameras
(scale= / trans2d=) and the point-light render_rgb are visualisation only and raise NotImplementedError.
"""
import pickle

import numpy as np
import torch

from .. import _capi

NV_HAND = 778
NV, NF = 2 * NV_HAND, 3076
MIN_SIZE, MAX_SIZE = 16, 1024


def two_hand_faces(right_faces):
    """vis_utils.py:262-265 from the right layer's faces (ManoLayer.get_faces(), [1538,3]): left = right faces with columns [1, 0, 2],
    right = right faces + 778 -> int32 [3076,3] on the host.  The indices are checked here, once: ValueError outside 0..777."""
    rf = np.asarray(right_faces)
    if rf.shape != (NF // 2, 3) or not np.issubdtype(rf.dtype, np.integer):
        raise ValueError('two_hand_faces: need integer right-hand faces [%d,3], got %s %s' % (NF // 2, rf.dtype, rf.shape))
    if rf.min() < 0 or rf.max() >= NV_HAND:
        raise ValueError('two_hand_faces: face index outside 0..%d (%d..%d)' % (NV_HAND - 1, rf.min(), rf.max()))
    rf = rf.astype(np.int64)
    return np.ascontiguousarray(np.concatenate([rf[:, [1, 0, 2]], rf + NV_HAND]).astype(np.int32))


def faces_from_layers(mano_layer):
    """two_hand_faces of the right GT layer's faces (dataset.gt_layers_from_checkpoint); a layer built from a checkpoint without
    th_faces carries all-zero faces, which render nothing: ValueError"""
    rf = np.asarray(mano_layer['right'].get_faces())
    if rf.size == 0 or not rf.any():
        raise ValueError('the right MANO layer has no faces (a checkpoint without init_regressor.mano_layer_right.th_faces?): '
                         'rendering needs the real face table')
    return two_hand_faces(rf)


def load_dense_colors(dense):
    """get_dense_color_path()'s table (a path to the pickle, or the [778,3] array in 0..1) -> float32 [1556,3] on the 0..255 scale:
    x 255 in float64, then float32 (vis_utils.py:343-354: torch.from_numpy(dense_coor) * 255, .to(v3d)), the same table for both hands"""
    if isinstance(dense, str):
        with open(dense, 'rb') as f:
            dense = pickle.load(f)
    d = np.asarray(dense, np.float64)
    if d.shape != (NV_HAND, 3):
        raise ValueError('dense colour table must be [%d,3], got %s' % (NV_HAND, d.shape))
    d = (d * 255).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([d, d]))


def mask_colors():
    """vis_utils.py:332-336: left vertices (0, 0, 255), right vertices (0, 255, 0), float32 [1556,3]"""
    c = np.zeros((NV, 3), np.float32)
    c[:NV_HAND, 2] = 255
    c[NV_HAND:, 1] = 255
    return c


def _check(t, dtype, shape, what):
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous() or not t.is_cuda:
        got = (t.dtype, tuple(t.shape), t.device) if isinstance(t, torch.Tensor) else type(t)
        raise ValueError('%s: need a contiguous %s cuda tensor %s, got %s' % (what, dtype, tuple(shape), got))


OUTPUTS = ('pix_to_face', 'zbuf', 'bary', 'mask', 'color_u8', 'color_f32')


def rasterize(verts, faces, K, S, colors=None, outputs=('pix_to_face', 'zbuf', 'bary'), workspace=None):
    """dir_render_two_hands: verts float32 cuda [B,1556,3] (left 0..777, right 778..1555, camera frame), faces int32 cuda [3076,3]
    (two_hand_faces), K float32 cuda [B,3,3], S in 16..1024, colors float32 cuda [1556,3] (0..255, needed by color_u8 / color_f32).
    outputs: any of pix_to_face int32 [B,S,S] (-1 background), zbuf float32 [B,S,S] (-1), bary float32 [B,S,S,3] (-1), mask uint8
    [B,S,S,3], color_u8 uint8 [B,S,S,3] (the frames cv.imwrite receives), color_f32 float32 [B,S,S,3] (texel / 255).  -> dict."""
    outputs = tuple(outputs)
    bad = [o for o in outputs if o not in OUTPUTS]
    if bad or not outputs:
        raise ValueError('rasterize: outputs must be a non-empty subset of %s, got %s' % (OUTPUTS, outputs))
    if not isinstance(S, int) or not MIN_SIZE <= S <= MAX_SIZE:
        raise ValueError('rasterize: S must be an int in %d..%d, got %r' % (MIN_SIZE, MAX_SIZE, S))
    B = verts.shape[0] if isinstance(verts, torch.Tensor) and verts.dim() == 3 else -1
    _check(verts, torch.float32, (B, NV, 3), 'rasterize: verts')
    _check(faces, torch.int32, (NF, 3), 'rasterize: faces')
    _check(K, torch.float32, (B, 3, 3), 'rasterize: K')
    if colors is not None:
        _check(colors, torch.float32, (NV, 3), 'rasterize: colors')
    elif 'color_u8' in outputs or 'color_f32' in outputs:
        raise ValueError('rasterize: color_u8 / color_f32 need `colors`')
    dev = verts.device
    out = {}
    for o in outputs:
        shape = (B, S, S) if o in ('pix_to_face', 'zbuf') else (B, S, S, 3)
        dt = {'pix_to_face': torch.int32, 'mask': torch.uint8, 'color_u8': torch.uint8}.get(o, torch.float32)
        out[o] = torch.empty(shape, dtype=dt, device=dev)
    if B == 0:
        return out
    L = _capi.lib()
    nbytes = int(L.dir_render_workspace_bytes(B))
    if workspace is None or workspace.numel() < nbytes:
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    P = _capi.ptr
    with torch.cuda.device(dev):
        _capi.check(L.dir_render_two_hands(P(verts), P(faces), P(K), P(colors), B, S, P(workspace), workspace.numel(),
                                           *[P(out.get(o)) for o in OUTPUTS], _capi.stream_ptr()), 'dir_render_two_hands')
    return out


def render_frames(verts, faces, K, dense_colors, S=256, workspace=None):
    """render_data's two frames for a batch: (mask, dense) uint8 cuda [B,S,S,3], in the renderer's array channel order -- what
    cv.imwrite receives (prepare_data.py:206-214) and what cv.imread / decode_bgr gives back (up to the JPEG round trip)"""
    o = rasterize(verts, faces, K, S, colors=dense_colors, outputs=('mask', 'color_u8'), workspace=workspace)
    return o['mask'], o['color_u8']


class mano_two_hands_renderer(object):
    """utils/vis_utils.py:mano_two_hands_renderer for the `cameras=` path on the GPU.

        r = mano_two_hands_renderer(right_faces=ManoLayer.get_faces(), dense_color=table, img_size=256, device='cuda')
        mask = r.render_mask(cameras=K, v3d_left=vl, v3d_right=vr)                 # [B,S,S,3] texel / 255
        img, alpha = r.render_densepose(cameras=K, v3d_left=vl, v3d_right=vr)      # [B,S,S,3], [B,S,S]
        depth = r.render_depth(cameras=K, v3d_left=vl, v3d_right=vr)               # [B,S,S,1], -1 background

    Built from the right layer's faces and the dense table (array [778,3] in 0..1 or the pickle's path), or, as the reference does, from
    mano_path ({'left', 'right'} MANO pickles; the right one's faces are used) and dense_path."""

    def __init__(self, mano_path=None, dense_path=None, img_size=224, device='cuda', right_faces=None, dense_color=None):
        if right_faces is None:
            if mano_path is None:
                raise ValueError('mano_two_hands_renderer: pass right_faces= (ManoLayer.get_faces()) or mano_path=')
            from ..models.manolayer import ManoLayer
            right_faces = ManoLayer(mano_path['right'], center_idx=None).get_faces()
        if dense_color is None:
            if dense_path is None:
                raise ValueError('mano_two_hands_renderer: pass dense_color= (the [778,3] table) or dense_path=')
            dense_color = dense_path
        if isinstance(img_size, tuple):
            raise NotImplementedError('mano_two_hands_renderer: only a square image size is supported')
        self.img_size = int(img_size)
        if not MIN_SIZE <= self.img_size <= MAX_SIZE:
            raise ValueError('mano_two_hands_renderer: img_size must be in %d..%d' % (MIN_SIZE, MAX_SIZE))
        self.device = torch.device(device)
        self.faces = torch.from_numpy(two_hand_faces(right_faces)).to(self.device)
        self.dense_coor = torch.from_numpy(load_dense_colors(dense_color)).to(self.device)
        self.mask_coor = torch.from_numpy(mask_colors()).to(self.device)

    def _raster(self, cameras, scale, trans2d, v3d_left, v3d_right, colors, outputs):
        if cameras is None or scale is not None or trans2d is not None:
            raise NotImplementedError('mano_two_hands_renderer: only the perspective cameras= path is built (orthographic scale= / '
                                      'trans2d= is visualisation only)')
        v3d = torch.cat((v3d_left, v3d_right), dim=1).to(self.device, torch.float32).contiguous()
        K = cameras.to(self.device, torch.float32).contiguous()
        return rasterize(v3d, self.faces, K, self.img_size, colors=colors, outputs=outputs)

    def render_mask(self, cameras=None, scale=None, trans2d=None, v3d_left=None, v3d_right=None):
        return self._raster(cameras, scale, trans2d, v3d_left, v3d_right, self.mask_coor, ('color_f32',))['color_f32']

    def render_densepose(self, cameras=None, scale=None, trans2d=None, v3d_left=None, v3d_right=None):
        o = self._raster(cameras, scale, trans2d, v3d_left, v3d_right, self.dense_coor, ('color_f32', 'pix_to_face'))
        return o['color_f32'], (o['pix_to_face'] >= 0).float()

    def render_depth(self, cameras=None, scale=None, trans2d=None, v3d_left=None, v3d_right=None):
        return self._raster(cameras, scale, trans2d, v3d_left, v3d_right, None, ('zbuf',))['zbuf'].unsqueeze(-1)

    def render_rgb(self, *args, **kwargs):
        raise NotImplementedError('mano_two_hands_renderer.render_rgb: point-light shading is visualisation only and not built')

    def render_rgb_orth(self, *args, **kwargs):
        raise NotImplementedError('mano_two_hands_renderer.render_rgb_orth: orthographic rendering is visualisation only and not built')
