"""numpy restatement of the shaded and orthographic two-hand renderer (dir_render_shaded in csrc/render.hip): pytorch3d's
verts_normals_packed, the OrthographicCameras of utils/vis_utils.py:138-149 and HardPhongShader with PointLights (default Materials and
BlendParams), float32 operation by operation.  Like raster_ref.py it loops over ALL faces in index order for every pixel, with no boxes
and no tiles, and the normals are a plain loop over the faces.  Written from the rules, not from the kernel; unpinned against pytorch3d,
which is not installed here -- and which composes its camera transforms as 4x4 matrix products, so even with it the agreement would be
to rounding, not to the bit.  Only + - * /, sqrt and compares are used; max(x, m) is where(x > m, x, m)."""
import numpy as np

import raster_ref as R

NV, NF = R.NV, R.NF
f32 = np.float32
EPS_N = f32(1e-6)

POINT_LIGHT = dict(ambient=(0.5, 0.5, 0.5), diffuse=(0.3, 0.3, 0.3), specular=(0.2, 0.2, 0.2), location=(0.0, 0.0, -1.0))
AMBIENT_LIGHT = dict(ambient=(1.0, 1.0, 1.0), diffuse=(0.0, 0.0, 0.0), specular=(0.0, 0.0, 0.0), location=(0.0, 0.0, 0.0))


def _max(x, m):
    return np.where(x > m, x, m).astype(np.float32)


def normalize(v, eps=EPS_N):
    """v [...,3] float32 -> v / max(sqrt(x*x + y*y + z*z), eps), the sum taken left to right"""
    v = np.asarray(v, np.float32)
    with np.errstate(all='ignore'):
        n = np.sqrt(v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1] + v[..., 2] * v[..., 2])
        return v / _max(n, eps)[..., None]


def cross(u, w):
    return np.array([u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]], np.float32)


def vertex_normals(verts, faces):
    """one mesh: verts float32 [V,3], faces int [F,3] -> float32 [V,3].  Faces are visited in ascending index; corner 0 adds
    cross(v1-v0, v2-v0) to its vertex, corner 1 cross(v2-v1, v0-v1), corner 2 cross(v0-v2, v1-v2); a face with an index outside the
    table adds nothing.  As every vertex's sum only ever receives its own faces in this order, it is the per-vertex ascending gather."""
    v = np.asarray(verts, np.float32)
    n = np.zeros_like(v)
    with np.errstate(all='ignore'):
        for f in np.asarray(faces, np.int64):
            if not all(0 <= i < len(v) for i in f):
                continue
            i0, i1, i2 = f
            n[i0] = n[i0] + cross(v[i1] - v[i0], v[i2] - v[i0])
            n[i1] = n[i1] + cross(v[i2] - v[i1], v[i0] - v[i1])
            n[i2] = n[i2] + cross(v[i0] - v[i2], v[i1] - v[i2])
    return normalize(n)


def project_ortho(verts, scale, trans2d):
    """x_ndc = (2 scale) * (-X) + (-trans2d.x), y likewise, depth = Z + 10 (R = diag(-1,-1,1), T = (0,0,10), focal 2 scale, principal
    point -trans2d)"""
    v = np.asarray(verts, np.float32)
    f = f32(2) * f32(scale)
    t = np.asarray(trans2d, np.float32)
    return f * (-v[:, 0]) + (-t[0]), f * (-v[:, 1]) + (-t[1]), v[:, 2] + f32(10)


def rasterize_ortho(verts, faces, scale, trans2d, S):
    """raster_ref.rasterize under the orthographic camera: no perspective correction (b_i = w_i, pz = w0 z0 + w1 z1 + w2 z2); the edge
    function, the zero-area skip, strict coverage, the pz < 0 skip, the depth tie and the pixel centres are the same"""
    x, y, z = project_ortho(verts, scale, trans2d)
    xs, ys = R.pixel_centres(S)
    PX = np.broadcast_to(xs[None, :], (S, S))
    PY = np.broadcast_to(ys[:, None], (S, S))
    best = np.full((S, S), -1, np.int32)
    bz = np.zeros((S, S), np.float32)
    bb = np.zeros((S, S, 3), np.float32)
    faces = np.asarray(faces, np.int64)
    with np.errstate(all='ignore'):
        for f in range(len(faces)):
            i0, i1, i2 = faces[f]
            if not all(0 <= i < len(x) for i in (i0, i1, i2)):
                continue
            x0, y0, z0, x1, y1, z1, x2, y2, z2 = x[i0], y[i0], z[i0], x[i1], y[i1], z[i1], x[i2], y[i2], z[i2]
            if np.abs(R.edge(x0, y0, x1, y1, x2, y2)) <= R.EPS:
                continue
            area = R.edge(x2, y2, x0, y0, x1, y1) + R.EPS
            b0 = R.edge(PX, PY, x1, y1, x2, y2) / area
            b1 = R.edge(PX, PY, x2, y2, x0, y0) / area
            b2 = R.edge(PX, PY, x0, y0, x1, y1) / area
            pz = b0 * z0 + b1 * z1 + b2 * z2
            take = (b0 > 0) & (b1 > 0) & (b2 > 0) & ~(pz < 0) & ((best < 0) | (pz < bz))
            best[take] = f
            bz[take] = pz[take]
            bb[take] = np.stack([b0, b1, b2], -1)[take]
    bg = best < 0
    bz[bg] = -1
    bb[bg] = -1
    return best, bz, bb


def interpolate(p2f, bary, faces, attr):
    """b0 a0 + b1 a1 + b2 a2 per component, left to right, for the covered pixels (others: whatever face 0 gives; masked by the caller)"""
    attr = np.asarray(attr, np.float32)
    vi = np.asarray(faces, np.int64)[np.where(p2f >= 0, p2f, 0)]
    b = bary.astype(np.float32)
    with np.errstate(all='ignore'):
        return b[..., 0:1] * attr[vi[..., 0]] + b[..., 1:2] * attr[vi[..., 1]] + b[..., 2:3] * attr[vi[..., 2]]


def dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def phong(p2f, bary, faces, verts, normals, colors, lights, centre):
    """HardPhongShader with one point light -> colour float32 [S,S,3] on the 0..255 scale of `colors`; background 1.0"""
    amb, dif, spe = (np.asarray(lights[k], np.float32) for k in ('ambient', 'diffuse', 'specular'))
    loc = np.asarray(lights['location'], np.float32)
    centre = np.asarray(centre, np.float32)
    fg = p2f >= 0
    with np.errstate(all='ignore'):
        p = interpolate(p2f, bary, faces, verts)
        n = normalize(interpolate(p2f, bary, faces, normals))
        d = normalize(loc - p)
        c = dot(n, d)
        diffuse = np.where(c > 0, c, f32(0)).astype(np.float32)
        view = normalize(centre - p)
        r = -d + f32(2) * (c[..., None] * n)
        vr = dot(view, r)
        a = np.where(c > 0, np.where(vr > 0, vr, f32(0)), f32(0)).astype(np.float32)
        for _ in range(6):
            a = a * a
        t = R.texel(p2f, bary, faces, colors)
        col = (amb + dif * diffuse[..., None]) * t + spe * a[..., None]
    col = col.astype(np.float32)
    col[~fg] = f32(1)
    return col


def render(verts, faces, S, colors, K=None, scale=None, trans2d=None, lights=POINT_LIGHT, background=None, normals=None):
    """one image -> dict of pix_to_face, zbuf, bary, normals, shaded_f32 (colour / 255), overlay_u8"""
    assert (K is None) != (scale is None)
    if K is not None:
        p2f, zb, ba = R.rasterize(verts, faces, K, S)
        centre = (0.0, 0.0, 0.0)
    else:
        p2f, zb, ba = rasterize_ortho(verts, faces, scale, trans2d, S)
        centre = (0.0, 0.0, -10.0)
    if normals is None:
        normals = vertex_normals(verts, faces)
    col = phong(p2f, ba, faces, np.asarray(verts, np.float32), normals, colors, lights, centre)
    ov = R.frame_u8(col)
    if background is not None:
        ov = np.where((p2f >= 0)[..., None], ov, np.asarray(background, np.uint8))
    return {'pix_to_face': p2f, 'zbuf': zb, 'bary': ba, 'normals': normals, 'shaded_f32': col / f32(255), 'overlay_u8': ov}


def remap_right_hand(sl, tl, sr, tr, v_right):
    """render_rgb_orth (vis_utils.py:313-322), one image: s = sr / sl, d = -(tl - tr) / 2 / sl, v' = s v, xy' += d"""
    v = np.asarray(v_right)
    s = sr / sl
    d = -(np.asarray(tl) - np.asarray(tr)) / 2 / sl
    out = s * v
    out[:, :2] = out[:, :2] + d
    return out


def draw_joints(image, uv_left, uv_right, palette, joint_radius=3.0, bone_radius=1.0):
    """one picture uint8 [S,S,3] + joints [21,2] in -1..1 per hand -> uint8 [S,S,3].  The project's own rule (not OpenCV's): a joint sits at
    (uv + 1) * S / 2, pixel (c, r) has its centre at (c + 0.5, r + 0.5); cov = clamp(radius + 0.5 - dist, 0, 1); o = o + cov * (colour - o) in
    float32, left hand then right hand, each its 20 bones (bone j joins joint j, or the wrist when j % 4 == 0, to joint j + 1, in finger
    j // 4's colour) then its 21 joints (joint k > 0 in finger (k - 1) // 4's colour, the wrist in palette[0]); round half to even, clamp."""
    S = image.shape[0]
    pal = np.asarray(palette, np.float32)
    o = image.astype(np.float32)
    px = (np.arange(S, dtype=np.float32) + f32(0.5))[None, :]
    py = (np.arange(S, dtype=np.float32) + f32(0.5))[:, None]

    def clamp01(x):
        return np.where(x > 0, np.where(x < 1, x, f32(1)), f32(0)).astype(np.float32)

    def blend(o, dist, rad, colour):
        cov = clamp01(f32(rad) + f32(0.5) - dist)[..., None]
        return o + cov * (colour - o)
    with np.errstate(all='ignore'):
        for uv in (uv_left, uv_right):
            P = (np.asarray(uv, np.float32) + f32(1)) * f32(S) / f32(2)
            for j in range(20):
                a, b = P[j if j % 4 else 0], P[j + 1]
                abx, aby = b[0] - a[0], b[1] - a[1]
                l2 = abx * abx + aby * aby
                if l2 > 0:
                    t = clamp01(((px - a[0]) * abx + (py - a[1]) * aby) / l2)
                else:
                    t = np.zeros((S, S), np.float32)
                dx, dy = px - (a[0] + t * abx), py - (a[1] + t * aby)
                o = blend(o, np.sqrt(dx * dx + dy * dy), bone_radius, pal[1 + j // 4])
            for k in range(21):
                dx, dy = px - P[k][0], py - P[k][1]
                o = blend(o, np.sqrt(dx * dx + dy * dy), joint_radius, pal[1 + (k - 1) // 4 if k else 0])
        v = np.rint(o)
    return np.clip(np.nan_to_num(v, nan=0.0), 0, 255).astype(np.uint8)
