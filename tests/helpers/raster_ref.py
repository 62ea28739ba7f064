"""numpy restatement of the two-hand mesh rasteriser (csrc/render.hip): pytorch3d's rasterize_meshes with the reference's settings
(blur_radius 0, faces_per_pixel 1, perspective-correct barycentrics, no culling, no z clipping) and the HardPhongShader + AmbientLights
texel, float32 operation by operation.  A plain loop over ALL faces in index order for every pixel (vectorised over the pixels only):
no boxes, no tiles, so it checks the kernel's face filter independently.  Written from the rules, not from the kernel; unpinned against
pytorch3d, which is not installed here."""
import numpy as np

NV, NF = 1556, 3076
f32 = np.float32
EPS = f32(1e-8)


def camera(K, S):
    """vis_utils.py:149-156: fx = -K00*2/S, fy = -K11*2/S, px = -K02*2/S + 1, py = -K12*2/S + 1 (float32)"""
    K = np.asarray(K, np.float32)
    s = f32(S)
    return ((-K[0, 0]) * f32(2) / s, (-K[1, 1]) * f32(2) / s, (-K[0, 2]) * f32(2) / s + f32(1), (-K[1, 2]) * f32(2) / s + f32(1))


def project(verts, K, S):
    """camera-frame vertices [V,3] -> NDC x, y and the view depth z, float32 [V] each: x = (fx X + px Z) / Z, y = (fy Y + py Z) / Z"""
    fx, fy, px, py = camera(K, S)
    v = np.asarray(verts, np.float32)
    X, Y, Z = v[:, 0], v[:, 1], v[:, 2]
    with np.errstate(all='ignore'):
        return (fx * X + px * Z) / Z, (fy * Y + py * Z) / Z, Z.copy()


def pixel_centres(S):
    """column c samples x = 1 - (2c+1)/S, row r samples y = 1 - (2r+1)/S -> (x [S], y [S])"""
    i = np.arange(S)
    c = f32(1) - (2 * i + 1).astype(np.float32) / f32(S)
    return c, c.copy()


def edge(px, py, ax, ay, bx, by):
    return (px - ax) * (by - ay) - (py - ay) * (bx - ax)


def rasterize(verts, faces, K, S):
    """one image: verts float32 [1556,3] (camera frame), faces int [F,3], K [3,3] -> pix_to_face int32 [S,S] (-1 background),
    zbuf float32 [S,S] (-1), bary float32 [S,S,3] (-1).  A face with an index outside the vertex table is skipped."""
    x, y, z = project(verts, K, S)
    xs, ys = pixel_centres(S)
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
            if np.abs(edge(x0, y0, x1, y1, x2, y2)) <= EPS:                    # zero area (a NaN area is not skipped here)
                continue
            area = edge(x2, y2, x0, y0, x1, y1) + EPS
            w0 = edge(PX, PY, x1, y1, x2, y2) / area
            w1 = edge(PX, PY, x2, y2, x0, y0) / area
            w2 = edge(PX, PY, x0, y0, x1, y1) / area
            t0, t1, t2 = w0 * z1 * z2, z0 * w1 * z2, z0 * z1 * w2
            s = t0 + t1 + t2
            d = np.where(s > EPS, s, EPS)                                      # max(sum, 1e-8); a NaN sum gives 1e-8
            b0, b1, b2 = t0 / d, t1 / d, t2 / d
            pz = b0 * z0 + b1 * z1 + b2 * z2
            take = (b0 > 0) & (b1 > 0) & (b2 > 0) & ~(pz < 0) & ((best < 0) | (pz < bz))
            best[take] = f
            bz[take] = pz[take]
            bb[take] = np.stack([b0, b1, b2], -1)[take]
    bg = best < 0
    bz[bg] = -1
    bb[bg] = -1
    return best, bz, bb


def texel(p2f, bary, faces, colors):
    """HardPhongShader + AmbientLights: t = b0*c0 + b1*c1 + b2*c2 per channel, left to right; background 1.0.  float32 [S,S,3]"""
    colors = np.asarray(colors, np.float32)
    faces = np.asarray(faces, np.int64)
    fg = p2f >= 0
    vi = faces[np.where(fg, p2f, 0)]                                           # [S,S,3] vertex indices
    b = bary.astype(np.float32)
    t = b[..., 0:1] * colors[vi[..., 0]] + b[..., 1:2] * colors[vi[..., 1]] + b[..., 2:3] * colors[vi[..., 2]]
    t[~fg] = f32(1)
    return t.astype(np.float32)


def frame_u8(t):
    """the array cv.imwrite receives: round_half_even(fl32(fl32(t / 255) * 255)), saturated to [0, 255]"""
    with np.errstate(all='ignore'):
        v = np.rint((np.asarray(t, np.float32) / f32(255)) * f32(255))
    return np.clip(np.nan_to_num(v, nan=0.0), 0, 255).astype(np.uint8)


def mask_colors():
    """vis_utils.py:332-336: left vertices (0, 0, 255), right vertices (0, 255, 0), array channel order"""
    c = np.zeros((NV, 3), np.float32)
    c[:NV // 2, 2] = 255
    c[NV // 2:, 1] = 255
    return c


def two_hand_faces(right_faces):
    """vis_utils.py:262-265: left = right faces with columns [1, 0, 2], right = right faces + 778"""
    rf = np.asarray(right_faces, np.int64)
    return np.concatenate([rf[:, [1, 0, 2]], rf + NV // 2]).astype(np.int32)


def render(verts, faces, K, S, colors=None):
    """one image -> dict of pix_to_face, zbuf, bary, mask (uint8 frame), and with `colors` [1556,3]: color_u8, color_f32 (t / 255)"""
    p2f, zb, ba = rasterize(verts, faces, K, S)
    out = {'pix_to_face': p2f, 'zbuf': zb, 'bary': ba, 'mask': frame_u8(texel(p2f, ba, faces, mask_colors()))}
    if colors is not None:
        t = texel(p2f, ba, faces, colors)
        out['color_u8'] = frame_u8(t)
        out['color_f32'] = t / f32(255)
    return out
