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
(scale= / trans2d=) and the point-light render_rgb are visualisation only and raise NotImplementedError in that class; the subclass
below provides them.

Viewing predictions (dir_render_shaded; the rules are in csrc/render.hip as well):

  vertex_normals    verts + faces -> [B,1556,3], pytorch3d's verts_normals_packed summed in a fixed order
  rasterize_shaded  perspective (K) or orthographic (scale, trans2d) camera, point-light Phong shading, optional background frames ->
                    pix_to_face / zbuf / bary / shaded_f32 / overlay_u8
  mano_two_hands_shaded_renderer
                    the subclass with render_rgb, render_rgb_orth and the scale= / trans2d= cameras of every render_* method
  overlay_predictions
                    one stage of DIR.forward's output + the input frames -> the two predicted hands drawn over the frames

Parity of the shaded path: bit-exact with tests/helpers/shade_ref.py, again unpinned against pytorch3d.  One difference is known:
pytorch3d composes its camera transforms as 4x4 matrix products, so with it installed equality would be to rounding, not to the bit.
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


# ---- shaded and orthographic rendering (dir_render_shaded) ----

class Lights(object):
    """One light for the Phong epilogue: ambient / diffuse / specular colours (light colour x the default Materials' 1) per channel, the
    point light's location in world space, shininess (64 is the only value the kernel takes)."""

    def __init__(self, ambient, diffuse, specular, location=(0.0, 0.0, 0.0), shininess=64.0):
        def three(v):
            v = tuple(float(x) for x in (v if isinstance(v, (tuple, list)) else (v, v, v)))
            if len(v) != 3:
                raise ValueError('Lights: need a scalar or three values, got %r' % (v,))
            return v
        self.ambient, self.diffuse, self.specular, self.location = three(ambient), three(diffuse), three(specular), three(location)
        self.shininess = float(shininess)
        if self.shininess != 64.0:
            raise ValueError('Lights: shininess %g: only 64 is built (the power is six squarings)' % self.shininess)

    def struct(self):
        F3 = _capi.C.c_float * 3
        return _capi.RenderLights(F3(*self.ambient), F3(*self.diffuse), F3(*self.specular), F3(*self.location), self.shininess)


POINT_LIGHT = Lights(0.5, 0.3, 0.2, (0.0, 0.0, -1.0))     # PointLights(location=[[0, 0, -1]]) with its defaults (vis_utils.py:123)
AMBIENT_LIGHT = Lights(1.0, 0.0, 0.0)                     # AmbientLights: the texel itself

LEFT_COLOR, RIGHT_COLOR = (204.0, 153.0, 0.0), (102.0, 102.0, 255.0)       # render_rgb's default v_color (vis_utils.py:286-293)
SHADED_OUTPUTS = ('pix_to_face', 'zbuf', 'bary', 'shaded_f32', 'overlay_u8')


def default_colors():
    """render_rgb's default vertex colours, float32 [1556,3]"""
    c = np.empty((NV, 3), np.float32)
    c[:NV_HAND] = LEFT_COLOR
    c[NV_HAND:] = RIGHT_COLOR
    return c


def face_adjacency(faces):
    """dir_render_adjacency for a face table (int32 cuda [3076,3]): every vertex's incident (face, corner) pairs in ascending face
    index.  Made once per table: the result is kept on the tensor and made again only after the tensor was written to."""
    _check(faces, torch.int32, (NF, 3), 'face_adjacency: faces')
    kept = getattr(faces, '_dir_adjacency', None)
    if kept is not None and kept[0] == faces._version:
        return kept[1]
    L = _capi.lib()
    adj = torch.empty(int(L.dir_render_adjacency_bytes()), dtype=torch.uint8, device=faces.device)
    with torch.cuda.device(faces.device):
        _capi.check(L.dir_render_adjacency(_capi.ptr(faces), _capi.ptr(adj), adj.numel(), _capi.stream_ptr()), 'dir_render_adjacency')
    faces._dir_adjacency = (faces._version, adj)
    return adj


def vertex_normals(verts, faces):
    """pytorch3d's Meshes.verts_normals_packed for the two-hand table, in the frame of `verts`: float32 cuda [B,1556,3] + int32 cuda
    [3076,3] -> float32 [B,1556,3].  Every corner of every face adds its own cross product to its vertex, in ascending face index (pytorch3d
    scatters with atomics, in no fixed order); then n / max(|n|, 1e-6).  A vertex of no face, or of zero-area faces only, keeps a zero normal."""
    B = verts.shape[0] if isinstance(verts, torch.Tensor) and verts.dim() == 3 else -1
    _check(verts, torch.float32, (B, NV, 3), 'vertex_normals: verts')
    adj = face_adjacency(faces)
    out = torch.empty_like(verts)
    if B == 0:
        return out
    with torch.cuda.device(verts.device):
        _capi.check(_capi.lib().dir_render_vertex_normals(_capi.ptr(verts), _capi.ptr(faces), _capi.ptr(adj), B, _capi.ptr(out),
                                                          _capi.stream_ptr()), 'dir_render_vertex_normals')
    return out


def rasterize_shaded(verts, faces, S, colors=None, K=None, scale=None, trans2d=None, lights=POINT_LIGHT, background=None,
                     outputs=('shaded_f32',), workspace=None):
    """dir_render_shaded: verts / faces / colors as `rasterize`; the camera is K float32 cuda [B,3,3] (perspective) OR scale float32 cuda
    [B] + trans2d float32 cuda [B,2] (orthographic: x_ndc = -(2 scale x + trans2d.x), depth z + 10), exactly one kind; lights: a Lights;
    background: uint8 cuda [B,S,S,3] frames for overlay_u8, or None.  outputs: any of pix_to_face / zbuf / bary (as `rasterize`; plain
    barycentrics under the orthographic camera), shaded_f32 float32 [B,S,S,3] (colour / 255, background 1/255), overlay_u8 uint8
    [B,S,S,3] (the rounded colour over the background frames).  -> dict."""
    outputs = tuple(outputs)
    bad = [o for o in outputs if o not in SHADED_OUTPUTS]
    if bad or not outputs:
        raise ValueError('rasterize_shaded: outputs must be a non-empty subset of %s, got %s' % (SHADED_OUTPUTS, outputs))
    if not isinstance(S, int) or not MIN_SIZE <= S <= MAX_SIZE:
        raise ValueError('rasterize_shaded: S must be an int in %d..%d, got %r' % (MIN_SIZE, MAX_SIZE, S))
    ortho = scale is not None or trans2d is not None
    if ortho == (K is not None):
        raise ValueError('rasterize_shaded: give exactly one camera kind, K= or scale= + trans2d= (%s given)' % ('both' if ortho else 'none'))
    if ortho and (scale is None or trans2d is None):
        raise ValueError('rasterize_shaded: the orthographic camera needs both scale= and trans2d=')
    B = verts.shape[0] if isinstance(verts, torch.Tensor) and verts.dim() == 3 else -1
    _check(verts, torch.float32, (B, NV, 3), 'rasterize_shaded: verts')
    _check(faces, torch.int32, (NF, 3), 'rasterize_shaded: faces')
    if ortho:
        _check(scale, torch.float32, (B,), 'rasterize_shaded: scale')
        _check(trans2d, torch.float32, (B, 2), 'rasterize_shaded: trans2d')
    else:
        _check(K, torch.float32, (B, 3, 3), 'rasterize_shaded: K')
    shade = 'shaded_f32' in outputs or 'overlay_u8' in outputs
    if colors is not None:
        _check(colors, torch.float32, (NV, 3), 'rasterize_shaded: colors')
    elif shade:
        raise ValueError('rasterize_shaded: shaded_f32 / overlay_u8 need `colors`')
    if shade and not isinstance(lights, Lights):
        raise ValueError('rasterize_shaded: lights must be a Lights, got %r' % (lights,))
    if background is not None:
        if 'overlay_u8' not in outputs:
            raise ValueError('rasterize_shaded: background frames are read by overlay_u8 only')
        _check(background, torch.uint8, (B, S, S, 3), 'rasterize_shaded: background')
    dev = verts.device
    out = {}
    for o in outputs:
        shape = (B, S, S) if o in ('pix_to_face', 'zbuf') else (B, S, S, 3)
        out[o] = torch.empty(shape, dtype={'pix_to_face': torch.int32, 'overlay_u8': torch.uint8}.get(o, torch.float32), device=dev)
    if B == 0:
        return out
    L = _capi.lib()
    adj = face_adjacency(faces) if shade else None
    nbytes = int(L.dir_render_shaded_workspace_bytes(B))
    if workspace is None or workspace.numel() < nbytes:
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    P = _capi.ptr
    with torch.cuda.device(dev):
        _capi.check(L.dir_render_shaded(P(verts), P(faces), P(adj), P(K), P(scale), P(trans2d), P(colors if shade else None),
                                        lights.struct() if shade else None, P(background), B, S, P(workspace), workspace.numel(),
                                        *[P(out.get(o)) for o in SHADED_OUTPUTS], _capi.stream_ptr()), 'dir_render_shaded')
    return out


def remap_right_hand(scale_left, trans2d_left, scale_right, trans2d_right, v3d_right):
    """render_rgb_orth's change of camera (vis_utils.py:313-322): the right hand's vertices as the LEFT hand's orthographic camera must
    see them to land where the right camera puts them: s = sr / sl, d = -(tl - tr) / 2 / sl, v' = s v, then xy' += d.  -> new tensor"""
    s = (scale_right / scale_left).unsqueeze(-1).unsqueeze(-1)
    d = (-(trans2d_left - trans2d_right) / 2 / scale_left.unsqueeze(-1)).unsqueeze(1)
    v = s * v3d_right
    v[..., :2] = v[..., :2] + d
    return v


class mano_two_hands_shaded_renderer(mano_two_hands_renderer):
    """mano_two_hands_renderer plus what shows a prediction: render_rgb (point-light Phong shading), render_rgb_orth (both hands'
    weak-perspective cameras in one picture) and the orthographic scale= / trans2d= cameras in render_mask / render_densepose /
    render_depth.  Exactly one camera kind is given per call.  UV textures are not built (NotImplementedError)."""

    def __init__(self, *args, **kwargs):
        super(mano_two_hands_shaded_renderer, self).__init__(*args, **kwargs)
        self.rgb_coor = torch.from_numpy(default_colors()).to(self.device)

    def _camera(self, cameras, scale, trans2d):
        if (cameras is None) == (scale is None and trans2d is None):
            raise ValueError('mano_two_hands_shaded_renderer: give exactly one camera kind, cameras= or scale= + trans2d=')
        if cameras is not None:
            return {'K': cameras.to(self.device, torch.float32).contiguous()}
        if scale is None or trans2d is None:
            raise ValueError('mano_two_hands_shaded_renderer: the orthographic camera needs both scale= and trans2d=')
        return {'scale': scale.to(self.device, torch.float32).reshape(-1).contiguous(),
                'trans2d': trans2d.to(self.device, torch.float32).contiguous()}

    def _shade(self, cameras, scale, trans2d, v3d_left, v3d_right, colors, lights, outputs, background=None):
        v3d = torch.cat((v3d_left, v3d_right), dim=1).to(self.device, torch.float32).contiguous()
        return rasterize_shaded(v3d, self.faces, self.img_size, colors=colors, lights=lights, background=background, outputs=outputs,
                                **self._camera(cameras, scale, trans2d))

    def _raster(self, cameras, scale, trans2d, v3d_left, v3d_right, colors, outputs):
        if cameras is not None and scale is None and trans2d is None:
            return super(mano_two_hands_shaded_renderer, self)._raster(cameras, scale, trans2d, v3d_left, v3d_right, colors, outputs)
        # orthographic: the ambient light through the shaded entry point gives the same texel / 255
        names = {'color_f32': 'shaded_f32'}
        o = self._shade(cameras, scale, trans2d, v3d_left, v3d_right, colors, AMBIENT_LIGHT, tuple(names.get(k, k) for k in outputs))
        return {k: o[names.get(k, k)] for k in outputs}

    def _colors(self, v_color):
        if v_color is None:
            return self.rgb_coor
        c = v_color if isinstance(v_color, torch.Tensor) else torch.tensor(v_color)
        c = c.to(self.device, torch.float32)
        if c.dim() == 3 and c.shape[0] == 1:
            c = c[0]
        if c.dim() > 2:
            raise NotImplementedError('mano_two_hands_shaded_renderer: one colour table [1556,3] for the whole batch')
        return c.expand(NV, 3).contiguous()

    def render_rgb(self, cameras=None, scale=None, trans2d=None, v3d_left=None, v3d_right=None, uv_verts=None, uv_faces=None,
                   texture=None, v_color=None, amblights=False, lights=None):
        """-> (img [B,S,S,3] = colour / 255 with background 1 / 255, alpha [B,S,S] = 1 where a face covers the pixel)"""
        if uv_verts is not None or uv_faces is not None or texture is not None:
            raise NotImplementedError('mano_two_hands_shaded_renderer: UV textures are not built')
        if lights is None:
            lights = AMBIENT_LIGHT if amblights else POINT_LIGHT
        o = self._shade(cameras, scale, trans2d, v3d_left, v3d_right, self._colors(v_color), lights, ('shaded_f32', 'pix_to_face'))
        return o['shaded_f32'], (o['pix_to_face'] >= 0).float()

    def render_rgb_orth(self, scale_left=None, trans2d_left=None, scale_right=None, trans2d_right=None, v3d_left=None, v3d_right=None,
                        uv_verts=None, uv_faces=None, texture=None, v_color=None, amblights=False, lights=None):
        """both hands, each under its own weak-perspective camera, in one picture: the right hand is moved into the left camera
        (remap_right_hand), then render_rgb(scale=scale_left, trans2d=trans2d_left)"""
        v3d_right = remap_right_hand(scale_left, trans2d_left, scale_right, trans2d_right, v3d_right)
        return self.render_rgb(scale=scale_left, trans2d=trans2d_left, v3d_left=v3d_left, v3d_right=v3d_right, uv_verts=uv_verts,
                               uv_faces=uv_faces, texture=texture, v_color=v_color, amblights=amblights, lights=lights)

    def render_overlay(self, background, cameras=None, scale=None, trans2d=None, v3d_left=None, v3d_right=None, v_color=None,
                       amblights=False, lights=None):
        """render_rgb composited over uint8 frames [B,S,S,3] in one launch: the frame's bytes where no face covers the pixel, the rounded
        colour elsewhere.  The colours are taken in the frames' channel order.  -> uint8 [B,S,S,3]"""
        if lights is None:
            lights = AMBIENT_LIGHT if amblights else POINT_LIGHT
        bg = background.to(self.device).contiguous()
        return self._shade(cameras, scale, trans2d, v3d_left, v3d_right, self._colors(v_color), lights, ('overlay_u8',), bg)['overlay_u8']


def overlay_predictions(outs, frames_u8, renderer, v_color=None, lights=None):
    """One stage of DIR.forward's output (a dict with pd_mesh_xyz_left / right [B,778,3] and pd_proj_left / right [B,3] = scale and 2-D
    translation) drawn over the frames the network saw: uint8 cuda [B,S,S,3] with S = renderer.img_size -> uint8 [B,S,S,3].

    DIR projects with uv = s * xy + t (utils/utils.py:47-63, uv in -1..1 over the image).  The orthographic camera's focal length is
    2 * scale (vis_utils.py:144), so each hand's camera gets scale = s / 2 and trans2d = t: a vertex then lands on the pixel whose centre is
    its uv.  Both hands go into the left hand's camera as render_rgb_orth does.  v_color: one table [1556,3] in the frames' channel order;
    the default is render_rgb's colours reversed, for the BGR frames of cv.imread / DecodeRing."""
    scale, trans2d, vl, vr = prediction_camera(outs)
    if v_color is None:
        v_color = renderer.rgb_coor.flip(-1)
    return renderer.render_overlay(frames_u8, scale=scale, trans2d=trans2d, v3d_left=vl, v3d_right=vr, v_color=v_color, lights=lights)


def prediction_camera(outs):
    """the one orthographic camera overlay_predictions renders a stage dict with: (scale [B] = s_left / 2, trans2d [B,2] = t_left, the left
    vertices, the right vertices moved into the left camera)"""
    pl, pr = outs['pd_proj_left'].float(), outs['pd_proj_right'].float()
    vl, vr = outs['pd_mesh_xyz_left'].float(), outs['pd_mesh_xyz_right'].float()
    sl, tl, sr, tr = pl[:, 0] / 2, pl[:, 1:3], pr[:, 0] / 2, pr[:, 1:3]
    return sl.contiguous(), tl.contiguous(), vl, remap_right_hand(sl, tl, sr, tr, vr)


# wrist, thumb, index, middle, ring, little finger -- this project's own palette, in the channel order of the picture it is drawn on
JOINT_PALETTE = ((255.0, 255.0, 255.0), (60.0, 60.0, 230.0), (60.0, 200.0, 230.0), (80.0, 220.0, 80.0), (230.0, 180.0, 60.0), (220.0, 80.0, 200.0))


def draw_joints(image_u8, uv_left, uv_right, joint_radius=3.0, bone_radius=1.0):
    """dir_render_joints: the predicted 2-D joints (pd_joint_uv_left / right, [B,21,2] in -1..1) drawn over uint8 cuda pictures [B,S,S,3],
    in place; -> image_u8.  This is NOT OpenCV's drawing (train.py's vis() uses cv2 circles and lines, whose anti-aliasing is pinned
    nowhere) but a rule of this project's own, pinned to its numpy restatement only: a joint sits at (uv + 1) * S / 2 with pixel centres
    at half-integers; a disc of joint_radius or a bone of half-width bone_radius covers a pixel by clamp(radius + 0.5 - distance, 0, 1),
    and the primitives are blended in float32 in a fixed order (left hand then right, bones then joints) with JOINT_PALETTE."""
    B, S = (image_u8.shape[0], image_u8.shape[1]) if isinstance(image_u8, torch.Tensor) and image_u8.dim() == 4 else (-1, -1)
    _check(image_u8, torch.uint8, (B, S, S, 3), 'draw_joints: image')
    if not MIN_SIZE <= S <= MAX_SIZE:
        raise ValueError('draw_joints: S must be in %d..%d, got %d' % (MIN_SIZE, MAX_SIZE, S))
    uv = [u.to(image_u8.device, torch.float32).contiguous() for u in (uv_left, uv_right)]
    for u in uv:
        _check(u, torch.float32, (B, 21, 2), 'draw_joints: uv')
    if B:
        with torch.cuda.device(image_u8.device):
            _capi.check(_capi.lib().dir_render_joints(_capi.ptr(image_u8), _capi.ptr(uv[0]), _capi.ptr(uv[1]), B, S, float(joint_radius),
                                                      float(bone_radius), _capi.stream_ptr()), 'dir_render_joints')
    return image_u8
