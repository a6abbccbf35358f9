"""NumPy restatement of csrc/amvs_mesh.hip: TSDF integration and marching-tetrahedra extraction in the kernels'
float32 operation order and output order, so that the device volume and mesh can be compared bit for bit.

Grid point (i, j, k) sits at origin + (i, j, k) * voxel; arrays are indexed [k, j, i] (x fastest, as on the device).
The triangle table is built here from first principles (sign cases of a tetrahedron, wound by an orientation test)
rather than copied from the kernel source; the device mesh matching this one element for element pins both.
"""
import numpy as np

F32 = np.float32

# tetrahedron edges (local vertex pairs), as in the kernel
TET_EDGES = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
# Kuhn tetrahedra 0 -> c1 -> c2 -> 7 (corner bit 0 = +x, 1 = +y, 2 = +z), one per axis order
# (x,y,z) (x,z,y) (y,x,z) (y,z,x) (z,x,y) (z,y,x); the odd orders are negatively oriented
KUHN = [(0, 1, 3, 7), (0, 1, 5, 7), (0, 2, 3, 7), (0, 2, 6, 7), (0, 4, 5, 7), (0, 4, 6, 7)]
KUHN_FLIP = [False, True, True, False, False, True]


def build_tri_table():
    """Triangles (as tetrahedron edge indices) of the 16 sign cases (bit v = local vertex v has f < 0), wound for a
    positively oriented tetrahedron so that the normal points toward the f >= 0 vertices."""
    T = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float64)

    def edge(a, b):
        return TET_EDGES.index((min(a, b), max(a, b)))

    table = []
    for case in range(16):
        inside = [v for v in range(4) if case >> v & 1]
        outside = [v for v in range(4) if not case >> v & 1]
        tris = []
        if len(inside) in (1, 3):
            lone = inside[0] if len(inside) == 1 else outside[0]
            o = [v for v in range(4) if v != lone]
            tris = [[edge(lone, o[0]), edge(lone, o[1]), edge(lone, o[2])]]
        elif len(inside) == 2:
            (p, q), (r, s) = inside, outside
            tris = [[edge(p, r), edge(p, s), edge(q, s)], [edge(p, r), edge(q, s), edge(q, r)]]
        wound = []
        for tri in tris:
            P = [(T[TET_EDGES[e][0]] + T[TET_EDGES[e][1]]) / 2 for e in tri]
            side = np.linalg.det(np.stack([P[1] - P[0], P[2] - P[0], T[outside[0]] - P[0]]))
            assert abs(side) > 1e-9
            wound.append(tri if side > 0 else [tri[0], tri[2], tri[1]])
        table.append(wound)
    return table


TRI_TABLE = build_tri_table()


def grid_coords(origin, voxel, dims):
    """float32 X, Y, Z of every grid point, shape (nz, ny, nx)."""
    nx, ny, nz = (int(d) for d in dims)
    o = np.asarray(origin, F32)
    v = F32(voxel)
    i = np.arange(nx, dtype=np.int64).astype(F32)
    j = np.arange(ny, dtype=np.int64).astype(F32)
    k = np.arange(nz, dtype=np.int64).astype(F32)
    X = np.broadcast_to((o[0] + i * v)[None, None, :], (nz, ny, nx))
    Y = np.broadcast_to((o[1] + j * v)[None, :, None], (nz, ny, nx))
    Z = np.broadcast_to((o[2] + k * v)[:, None, None], (nz, ny, nx))
    return X, Y, Z


def integrate(depth, conf, colors_bgr, K, poses, min_views, origin, voxel, dims, trunc):
    """depth, conf: (n, H, W) float32; colors_bgr: (n, H, W, 3) uint8; K (3,3); poses: (n, 12) float32 (R row-major,
    t).  Returns tsdf (nz,ny,nx), weight (nz,ny,nx), color_sum (nz,ny,nx,3) RGB, all float32."""
    depth = np.asarray(depth, F32)
    conf = np.asarray(conf, F32)
    n, H, W = depth.shape
    Kf = np.asarray(K, F32).reshape(9)
    P = np.asarray(poses, F32).reshape(n, 12)
    X, Y, Z = grid_coords(origin, voxel, dims)
    mv, tr = F32(min_views), F32(trunc)
    s = np.zeros(X.shape, F32)
    w = np.zeros(X.shape, F32)
    csum = np.zeros(X.shape + (3,), F32)
    with np.errstate(all="ignore"):
        for m in range(n):
            R = P[m]
            zc = ((R[6] * X + R[7] * Y) + R[8] * Z) + R[11]
            xc = ((R[0] * X + R[1] * Y) + R[2] * Z) + R[9]
            yc = ((R[3] * X + R[4] * Y) + R[5] * Z) + R[10]
            pu = (Kf[0] * xc + Kf[1] * yc) + Kf[2] * zc
            pv = (Kf[3] * xc + Kf[4] * yc) + Kf[5] * zc
            pw = (Kf[6] * xc + Kf[7] * yc) + Kf[8] * zc
            fx = np.floor(pu / pw + F32(0.5))
            fy = np.floor(pv / pw + F32(0.5))
            ok = (zc > 0) & (fx >= 0) & (fx < F32(W)) & (fy >= 0) & (fy < F32(H))
            px = np.where(ok, fx, 0).astype(np.int64)
            py = np.where(ok, fy, 0).astype(np.int64)
            d = depth[m][py, px]
            c = conf[m][py, px]
            ok &= (d > 0) & (c >= mv)
            sdf = d - zc
            ok &= ~(sdf < -tr)
            val = np.minimum(F32(1), sdf / tr)
            s = np.where(ok, s + val, s)
            w = np.where(ok, w + F32(1), w)
            bgr = colors_bgr[m][py, px].astype(F32)
            for ch in range(3):
                csum[..., ch] = np.where(ok, csum[..., ch] + bgr[..., 2 - ch], csum[..., ch])
    with np.errstate(all="ignore"):
        tsdf = np.where(w > 0, s / w, F32(1)).astype(F32)
    return tsdf, w, csum


def _round_u8(c):
    return np.minimum(F32(255), np.maximum(F32(0), np.floor(c + F32(0.5)))).astype(np.uint8)


def extract(tsdf, weight, color_sum, origin, voxel):
    """Marching tetrahedra of the kernels, same order: vertices (V,3) float32, faces (F,3) int32, colours (V,3) uint8."""
    tsdf = np.asarray(tsdf, F32)
    weight = np.asarray(weight, F32)
    nz, ny, nx = tsdf.shape
    N = nx * ny * nz
    f = tsdf.reshape(N)
    w = weight.reshape(N)
    cs = np.asarray(color_sum, F32).reshape(N, 3)
    o = np.asarray(origin, F32)
    v = F32(voxel)
    p = np.arange(N)
    i, j, k = p % nx, (p // nx) % ny, p // (nx * ny)
    inside = f < 0
    obs = w > 0
    # (a) crossing edges: (N, 7) flags, direction d = 1 .. 7 in column d - 1
    cross = np.zeros((N, 7), bool)
    for d in range(1, 8):
        di, dj, dk = d & 1, (d >> 1) & 1, d >> 2
        inb = (i + di < nx) & (j + dj < ny) & (k + dk < nz)
        q = np.where(inb, p + di + nx * (dj + ny * dk), 0)
        cross[:, d - 1] = inb & obs & obs[q] & (inside != inside[q])
    vid = np.full((N, 7), -1, np.int64)
    pts, dirs = np.nonzero(cross)                       # point order, then direction order
    vid[pts, dirs] = np.arange(len(pts))
    d = dirs + 1
    di, dj, dk = d & 1, (d >> 1) & 1, d >> 2
    q = pts + di + nx * (dj + ny * dk)
    f0, f1 = f[pts], f[q]
    with np.errstate(all="ignore"):
        t = f0 / (f0 - f1)
    pi, pj, pk = i[pts], j[pts], k[pts]
    verts = np.empty((len(pts), 3), F32)
    for a, (g0, dg) in enumerate(((pi, di), (pj, dj), (pk, dk))):
        c0 = o[a] + g0.astype(F32) * v
        c1 = o[a] + (g0 + dg).astype(F32) * v
        verts[:, a] = c0 + t * (c1 - c0)
    with np.errstate(all="ignore"):
        m0 = cs[pts] / w[pts][:, None]
        m1 = cs[q] / w[q][:, None]
    colors = _round_u8(m0 + t[:, None] * (m1 - m0))
    # (b, c) faces of every interior cube, tetrahedron by tetrahedron, in table order
    interior = (i + 1 < nx) & (j + 1 < ny) & (k + 1 < nz)
    cubes = p[interior]
    corner_pt = [cubes + (c & 1) + nx * (((c >> 1) & 1) + ny * (c >> 2)) for c in range(8)]
    slots = []                                          # per (tet, triangle slot): (valid mask, (C, 3) ids)
    for t_idx, tet in enumerate(KUHN):
        ok = np.ones(len(cubes), bool)
        case = np.zeros(len(cubes), np.int64)
        for lv, c in enumerate(tet):
            ok &= obs[corner_pt[c]]
            case |= inside[corner_pt[c]].astype(np.int64) << lv
        for r in range(2):
            ids = np.full((len(cubes), 3), -1, np.int64)
            valid = np.zeros(len(cubes), bool)
            for cs_ in range(16):
                if r >= len(TRI_TABLE[cs_]):
                    continue
                sel = ok & (case == cs_)
                if not np.any(sel):
                    continue
                tri = TRI_TABLE[cs_][r]
                if KUHN_FLIP[t_idx]:
                    tri = [tri[0], tri[2], tri[1]]
                for e_i, te in enumerate(tri):
                    a, b = TET_EDGES[te]
                    ca, cb = tet[a], tet[b]
                    ids[sel, e_i] = vid[corner_pt[ca][sel], (ca ^ cb) - 1]
                valid |= sel
            slots.append((valid, ids))
    valid = np.stack([s[0] for s in slots], axis=1)                 # (C, 12): tet-major, then slot
    ids = np.stack([s[1] for s in slots], axis=1)                   # (C, 12, 3)
    faces = ids[valid]
    assert faces.size == 0 or faces.min() >= 0
    # (d) keep the vertices the faces use, in their order, and renumber the faces
    used = np.zeros(len(verts), bool)
    used[faces.reshape(-1)] = True
    new_id = np.cumsum(used) - 1
    return verts[used], new_id[faces].astype(np.int32).reshape(-1, 3), colors[used]

