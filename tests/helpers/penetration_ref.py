"""float64 numpy restatement of the inter-hand penetration measures (dir_amd/csrc/penetration.hip states the same rules), and the closed
meshes the tests put through both.  Nothing here is shared with the product code.

  valid_faces       faces without a repeated index and with every index in 0..V-1 (the others are skipped everywhere)
  winding           generalised winding number (Van Oosterom-Strackee solid angles; atan2(0, 0) counts as 0), chunked over the faces
  distance          min over the faces of the distance to the closest point of the closed triangle (Ericson 5.1.5)
  penetration       both directions: count / max_depth / sum_depth over the vertices with |w| > 0.5
  lattice           the float32 index ranges of the voxel lattice and its float32 points
  intersection      n_both / cells / volume
  octasphere, cube, open_hemisphere, open_cylinder     closed-form meshes
"""
import numpy as np

CHUNK = 256


def valid_faces(faces, n_verts):
    f = np.asarray(faces, np.int64)
    ok = ((f >= 0) & (f < n_verts)).all(1) & (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])
    return f[ok]


def winding(points, verts, faces, dtype=np.float64):
    p, v = np.asarray(points, dtype), np.asarray(verts, dtype)
    f = valid_faces(faces, len(v))
    total = np.zeros(len(p), dtype)
    for c0 in range(0, len(f), CHUNK):
        t = v[f[c0:c0 + CHUNK]]                                   # [F,3,3]
        a, b, c = (t[None, :, k] - p[:, None] for k in range(3))   # [P,F,3]
        la, lb, lc = (np.sqrt((x * x).sum(-1)) for x in (a, b, c))
        det = (a * np.cross(b, c)).sum(-1)
        den = la * lb * lc + (a * b).sum(-1) * lc + (b * c).sum(-1) * la + (c * a).sum(-1) * lb
        ang = np.arctan2(det, den)
        ang[(det == 0) & (den == 0)] = 0
        total += (2 * ang).sum(1, dtype=dtype)
    return total / dtype(4 * np.pi)


def _closest(p, a, b, c):
    """closest point of triangle (a, b, c) to p, all [..., 3]: the regions of Ericson 5.1.5, decided in the book's order"""
    ab, ac = b - a, c - a
    dot = lambda x, y: (x * y).sum(-1)  # noqa: E731
    d1, d2 = dot(ab, p - a), dot(ac, p - a)
    d3, d4 = dot(ab, p - b), dot(ac, p - b)
    d5, d6 = dot(ab, p - c), dot(ac, p - c)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    with np.errstate(divide='ignore', invalid='ignore'):
        safe = lambda n, d: np.where(d != 0, n / np.where(d != 0, d, 1), 0)  # noqa: E731
        t_ab, t_ac, t_bc = safe(d1, d1 - d3), safe(d2, d2 - d6), safe(d4 - d3, (d4 - d3) + (d5 - d6))
        s = va + vb + vc
        q_in = a + ab * safe(vb, s)[..., None] + ac * safe(vc, s)[..., None]
    conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (d6 >= 0) & (d5 <= d6),
             (vc <= 0) & (d1 >= 0) & (d3 <= 0), (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)]
    cands = [a, b, c, a + ab * t_ab[..., None], a + ac * t_ac[..., None], b + (c - b) * t_bc[..., None]]
    q, done = q_in, np.zeros(d1.shape, bool)
    for cond, cand in zip(conds, cands):
        take = cond & ~done
        q = np.where(take[..., None], cand, q)
        done |= cond
    return q


def distance(points, verts, faces, dtype=np.float64):
    p, v = np.asarray(points, dtype), np.asarray(verts, dtype)
    f = valid_faces(faces, len(v))
    best = np.full(len(p), np.inf, dtype)
    for c0 in range(0, len(f), CHUNK):
        t = v[f[c0:c0 + CHUNK]]
        pp = np.broadcast_to(p[:, None], (len(p), t.shape[0], 3))
        q = _closest(pp, *(np.broadcast_to(t[None, :, k], pp.shape) for k in range(3)))
        best = np.minimum(best, np.sqrt(((q - pp) ** 2).sum(-1)).min(1))
    return best


def penetration(verts_a, faces_a, verts_b, faces_b):
    """one sample -> {'winding', 'dist' [Va+Vb] (A's vertices against B first), 'count' [2], 'max_depth' [2], 'sum_depth' [2], 'depth'}"""
    w = np.concatenate([winding(verts_a, verts_b, faces_b), winding(verts_b, verts_a, faces_a)])
    d = np.concatenate([distance(verts_a, verts_b, faces_b), distance(verts_b, verts_a, faces_a)])
    return dict(aggregate(w, d, len(verts_a)), winding=w, dist=d)


def aggregate(w, d, n_a):
    inside = np.abs(w) > 0.5
    parts = [(inside[:n_a], d[:n_a]), (inside[n_a:], d[n_a:])]
    out = {'count': np.array([m.sum() for m, _ in parts]), 'max_depth': np.array([x[m].max() if m.any() else 0.0 for m, x in parts]),
           'sum_depth': np.array([x[m].sum(dtype=np.float64) for m, x in parts])}
    out['depth'] = out['max_depth'].max()
    return out


def lattice(verts_a, verts_b, h=0.005):
    """-> (first index [3], count [3], points float32 [n,3] in index order i, j, k with k fastest); float32 bounds and float32 division"""
    a, b, h = np.asarray(verts_a, np.float32), np.asarray(verts_b, np.float32), np.float32(h)
    lo, hi = np.maximum(a.min(0), b.min(0)), np.minimum(a.max(0), b.max(0))
    i0, i1 = np.ceil(lo / h).astype(np.int64), np.floor(hi / h).astype(np.int64)
    n = np.maximum(i1 - i0 + 1, 0)
    idx = np.stack(np.meshgrid(*(np.arange(i0[k], i0[k] + n[k]) for k in range(3)), indexing='ij'), -1).reshape(-1, 3)
    return i0, n, idx.astype(np.float32) * h


def intersection(verts_a, faces_a, verts_b, faces_b, h=0.005, max_cells=1 << 17):
    """one sample -> {'cells', 'n_both', 'volume', 'points' float32 [cells,3], 'w_a', 'w_b' float64 [cells]} (w_b is computed everywhere)"""
    i0, n, pts = lattice(verts_a, verts_b, h)
    cells = int(np.prod(n))
    if cells > max_cells:
        return {'cells': cells, 'n_both': 0, 'volume': float('nan')}
    wa, wb = winding(pts, verts_a, faces_a), winding(pts, verts_b, faces_b)
    both = (np.abs(wa) > 0.5) & (np.abs(wb) > 0.5)
    return {'cells': cells, 'n_both': int(both.sum()), 'volume': float(both.sum()) * float(h) ** 3, 'points': pts, 'w_a': wa, 'w_b': wb}


# ---------------------------------------------------------------------------------------------------------------- closed-form meshes
def octasphere(subdiv=3, radius=1.0, centre=(0, 0, 0)):
    """octahedron subdivided `subdiv` times, every vertex pushed to the sphere; outward faces.  subdiv 3: 258 vertices, 512 faces"""
    v = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    f = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    v = [np.array(x, np.float64) for x in v]
    for _ in range(subdiv):
        mid, nf = {}, []

        def m(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                x = v[i] + v[j]
                v.append(x / np.linalg.norm(x))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca)]
        f = nf
    return np.array(v) * radius + np.asarray(centre, np.float64), np.array(f, np.int32)


def cube(half=1.0, centre=(0, 0, 0)):
    """axis-aligned cube [-half, half]^3 + centre, 8 vertices, 12 outward triangles"""
    v = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float64) * half + np.asarray(centre, np.float64)
    q = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    f = [t for a, b, c, d in q for t in ((a, b, c), (a, c, d))]
    return v, np.array(f, np.int32)


def cube_distance(p, half=1.0, centre=(0, 0, 0)):
    """distance from p [N,3] to the SURFACE of the cube"""
    q = np.abs(np.asarray(p, np.float64) - np.asarray(centre, np.float64)) - half
    outside = np.sqrt((np.maximum(q, 0) ** 2).sum(-1))
    return np.where((q <= 0).all(-1), -q.max(-1), outside)


def open_hemisphere(subdiv=3, radius=1.0):
    """the z >= 0 half of the octasphere: its boundary is the equator, one simple loop"""
    v, f = octasphere(subdiv, radius)
    keep = (v[f][:, :, 2] >= -1e-12).all(1)
    return _compact(v, f[keep])


def open_cylinder(n=24, radius=1.0, height=2.0):
    """a tube closed at the bottom by a fan around a centre vertex, open at the top: one boundary loop of n vertices"""
    ang = 2 * np.pi * np.arange(n) / n
    ring = np.stack([radius * np.cos(ang), radius * np.sin(ang)], 1)
    v = np.concatenate([np.c_[ring, np.zeros(n)], np.c_[ring, np.full(n, height)], [[0, 0, 0]]])
    f = []
    for i in range(n):
        j = (i + 1) % n
        f += [(i, j, n + j), (i, n + j, n + i), (2 * n, j, i)]
    return v, np.array(f, np.int32)


def _compact(v, f):
    used = np.unique(f)
    remap = np.full(len(v), -1, np.int64)
    remap[used] = np.arange(len(used))
    return v[used], remap[f].astype(np.int32)


def hand_pairs(n_pairs=6, seed=0, noise=0.003, offset=0.02):
    """pairs from the synthetic MANO table: the right template (+ per-vertex noise), its mirror in x (+ noise) shifted by a random offset ->
    (verts_a float32 [n,778,3], faces_a int32 [1538,3], verts_b, faces_b)"""
    from dir_amd import synth
    t = synth.synthetic_mano_tables('right')
    tpl, faces = np.asarray(t['v_template'], np.float64), np.asarray(t['f']).astype(np.int32)
    g = np.random.default_rng(seed)
    a = tpl[None] + g.normal(0, noise, (n_pairs,) + tpl.shape)
    b = tpl[None] * np.array([-1.0, 1.0, 1.0]) + g.normal(0, noise, (n_pairs,) + tpl.shape) + g.normal(0, offset, (n_pairs, 1, 3))
    return a.astype(np.float32), faces, b.astype(np.float32), np.ascontiguousarray(faces[:, [1, 0, 2]])
