"""numpy restatement of the mesh renderer (csrc/render.hip): the truth the renderer tests compare against.

The vertex stage runs in the dtype asked for: float64 is the truth, float32 (the same operations in the same order) is the
yardstick the bounds are taken from.  The raster stage takes fp32 screen coordinates, snaps them with the kernel's
rint(x * 256) and decides coverage with exact int64 edge functions and the top-left rule, so coverage has no tolerance; depth and
shading run in the dtype asked for.  Each face is restricted to its bounding box, so a FLAME-sized mesh takes seconds.
Nothing in the product imports this file.
"""
import numpy as np

U = 2.0 ** -24
SNAP_LIMIT = 2.0 ** 30


def rel_err(g, g64):
    """|g - g64| / max(1, |g64|) per element."""
    g64 = np.asarray(g64, np.float64)
    return np.abs(np.asarray(g, np.float64) - g64) / np.maximum(1.0, np.abs(g64))


def bound(yardstick, g64, u=U):
    """max(16 u, 4 x the float32 restatement's own worst error against float64)."""
    e = rel_err(yardstick, g64)
    return max(16.0 * u, 4.0 * (float(e.max()) if e.size else 0.0))


def rodrigues(r, dtype=np.float64):
    """cv2.Rodrigues' rotation matrix: angle = |r|, identity at 0."""
    r = np.asarray(r, dtype).reshape(3)
    th = np.sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2])
    if not th > 0:
        return np.eye(3, dtype=dtype)
    k = r / th
    s, c = np.sin(th), np.cos(th)
    c1 = dtype(1) - c
    return np.array([[c + c1 * k[0] * k[0], c1 * k[0] * k[1] - s * k[2], c1 * k[0] * k[2] + s * k[1]],
                     [c1 * k[0] * k[1] + s * k[2], c + c1 * k[1] * k[1], c1 * k[1] * k[2] - s * k[0]],
                     [c1 * k[0] * k[2] - s * k[1], c1 * k[1] * k[2] + s * k[0], c + c1 * k[2] * k[2]]], dtype=dtype)


def _unit_or_z(n):
    n2 = (n * n).sum(-1, keepdims=True)
    ok = n2 > 0
    out = n / np.sqrt(np.where(ok, n2, 1))
    return np.where(ok, out, np.array([0, 0, 1], n.dtype))


def vertex_normals(verts, faces, dtype=np.float64):
    """Area-weighted unit vertex normals of one frame (V, 3): the incident faces' un-normalised cross products summed in
    ascending face order (np.add.at works through its indices in order), a face once per vertex; zero sum -> (0, 0, 1)."""
    v = np.asarray(verts).astype(dtype)
    f = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    cr = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]).astype(dtype)
    n = np.zeros_like(v)
    np.add.at(n, f[:, 0], cr)
    np.add.at(n, f[:, 1], np.where((f[:, 1] != f[:, 0])[:, None], cr, 0).astype(dtype))
    np.add.at(n, f[:, 2], np.where(((f[:, 2] != f[:, 0]) & (f[:, 2] != f[:, 1]))[:, None], cr, 0).astype(dtype))
    return _unit_or_z(n)


def vertex_stage(verts, faces, view, focal, height, width, t_center=None, rot=None, dtype=np.float64):
    """verts (B, V, 3), view (3, 4) world -> eye, rot (B, 3) or None -> (screen (B, V, 3) = (x_s, y_s, d), normals (B, V, 3))."""
    verts = np.asarray(verts)
    view = np.asarray(view).astype(dtype)
    focal, Wf, Hf, half = dtype(np.float32(focal)), dtype(width), dtype(height), dtype(0.5)
    screen, normals = [], []
    for b in range(verts.shape[0]):
        p = verts[b].astype(dtype)
        n = vertex_normals(verts[b], faces, dtype)
        if rot is not None:
            R = rodrigues(np.asarray(rot)[b].astype(np.float32), dtype)
            tc = np.asarray(t_center).astype(np.float32).astype(dtype)
            p = (p - tc) @ R.T + tc
            n = n @ R.T
        pe = p @ view[:, :3].T + view[:, 3]
        ne = n @ view[:, :3].T
        d = -pe[:, 2]
        xn, yn = focal * pe[:, 0] / d, focal * pe[:, 1] / d
        screen.append(np.stack([(xn * half + half) * Wf, (half - yn * half) * Hf, d], axis=-1).astype(dtype))
        normals.append(ne.astype(dtype))
    return np.stack(screen), np.stack(normals)


def _edge(ax, ay, bx, by, px, py):
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax)


def _top_left(ax, ay, bx, by):
    dx, dy = bx - ax, by - ay
    return (dy > 0) | ((dy == 0) & (dx > 0))


def face_table(screen, faces, near):
    """Per-face set-up of one frame, as the kernel's face_setup makes it: snapped int64 coordinates oriented to a positive
    doubled area (vertices 1 and 2 swapped where it was negative), vertex ids in that order, eye depths, and `ok`."""
    s = np.asarray(screen, np.float32)
    f = np.asarray(faces).astype(np.int64).reshape(-1, 3).copy()
    V = s.shape[0]
    ok = ((f >= 0) & (f < V)).all(1)
    f[~ok] = 0
    d = s[f, 2]                                                   # (F, 3) float32
    with np.errstate(invalid="ignore", over="ignore"):
        ok &= (d >= np.float32(near)).all(1)
        X, Y = np.rint(s[f, 0] * np.float32(256)), np.rint(s[f, 1] * np.float32(256))
        ok &= (np.abs(X) < SNAP_LIMIT).all(1) & (np.abs(Y) < SNAP_LIMIT).all(1)
    X = np.where(ok[:, None], X, 0).astype(np.int64)
    Y = np.where(ok[:, None], Y, 0).astype(np.int64)
    area = _edge(X[:, 0], Y[:, 0], X[:, 1], Y[:, 1], X[:, 2], Y[:, 2])
    ok &= area != 0
    flip = area < 0
    for a in (X, Y, f, d):
        a[flip, 1], a[flip, 2] = a[flip, 2].copy(), a[flip, 1].copy()
    return dict(X=X, Y=Y, ids=f, d=d, area=np.abs(area), ok=ok)


def raster_stage(screen, normals, faces, height, width, near, far, shade, lights, background, dtype=np.float64, fill_rule=True):
    """One frame.  screen / normals (V, 3) fp32 (the vertex stage's outputs).  Returns a dict: color (H, W, 3) in `dtype` before
    quantisation, color_u8 (H, W, 3), depth (H, W) (0 = background), face_id (H, W) int32 (-1 = background), depth2 (H, W) the
    second-nearest fragment's depth (inf where there is none), count (H, W) how many faces cover the pixel centre."""
    H, W = int(height), int(width)
    t = face_table(screen, faces, near)
    X, Y, area = t["X"], t["Y"], t["area"]
    q = dtype(1) / t["d"].astype(dtype)
    d1 = np.full((H, W), np.inf, dtype)
    d2 = np.full((H, W), np.inf, dtype)
    fid = np.full((H, W), -1, np.int32)
    count = np.zeros((H, W), np.int32)
    jlo = np.maximum((X.min(1) + 127) >> 8, 0)
    jhi = np.minimum((X.max(1) - 128) >> 8, W - 1)
    ilo = np.maximum((Y.min(1) + 127) >> 8, 0)
    ihi = np.minimum((Y.max(1) - 128) >> 8, H - 1)
    live = np.nonzero(t["ok"] & (jlo <= jhi) & (ilo <= ihi))[0]

    def weights(f, px, py):
        e0 = _edge(X[f, 1], Y[f, 1], X[f, 2], Y[f, 2], px, py)
        e1 = _edge(X[f, 2], Y[f, 2], X[f, 0], Y[f, 0], px, py)
        e2 = _edge(X[f, 0], Y[f, 0], X[f, 1], Y[f, 1], px, py)
        A = area[f].astype(dtype)
        w0, w1, w2 = e0.astype(dtype) / A, e1.astype(dtype) / A, e2.astype(dtype) / A
        iz = (w0 * q[f, 0] + w1 * q[f, 1]) + w2 * q[f, 2]
        return (e0, e1, e2), (w0, w1, w2), iz

    for f in live:
        py, px = np.meshgrid(256 * np.arange(ilo[f], ihi[f] + 1, dtype=np.int64) + 128,
                             256 * np.arange(jlo[f], jhi[f] + 1, dtype=np.int64) + 128, indexing="ij")
        e, _, iz = weights(f, px, py)
        inside = np.ones(px.shape, bool)
        for k, (a, b) in enumerate(((1, 2), (2, 0), (0, 1))):
            keep_zero = bool(_top_left(X[f, a], Y[f, a], X[f, b], Y[f, b])) if fill_rule else True
            inside &= (e[k] > 0) | ((e[k] == 0) & keep_zero)
        with np.errstate(divide="ignore"):
            d = dtype(1) / iz
        inside &= (d >= dtype(near)) & (d <= dtype(far))
        if not inside.any():
            continue
        win = (slice(ilo[f], ihi[f] + 1), slice(jlo[f], jhi[f] + 1))
        count[win] += inside
        c1, c2, cf = d1[win], d2[win], fid[win]
        nearer = inside & (d < c1)               # faces come in ascending order: on a tie the lower id stays
        other = inside & ~nearer
        c2[nearer] = c1[nearer]
        c1[nearer] = d[nearer]
        cf[nearer] = f
        c2[other] = np.minimum(c2[other], d[other])

    covered = fid >= 0
    ii, jj = np.nonzero(covered)
    f = fid[ii, jj].astype(np.int64)
    _, w, iz = weights(f, 256 * jj.astype(np.int64) + 128, 256 * ii.astype(np.int64) + 128)
    nv = np.asarray(normals, np.float32).astype(dtype)[t["ids"][f]]                  # (P, 3 vertices, 3)
    p = [w[k] * q[f, k] / iz for k in range(3)]
    n = _unit_or_z(p[0][:, None] * nv[:, 0] + p[1][:, None] * nv[:, 1] + p[2][:, None] * nv[:, 2])
    shade = np.asarray(shade, np.float32).astype(dtype)
    lights = np.asarray(lights, np.float32).astype(dtype).reshape(-1, 4)
    diff = np.zeros(n.shape[0], dtype)
    for k in range(lights.shape[0]):
        diff = diff + lights[k, 3] * np.maximum(dtype(0), n[:, 0] * lights[k, 0] + n[:, 1] * lights[k, 1] + n[:, 2] * lights[k, 2])
    diff = diff * dtype(np.float32(0.318309886183790672))
    c = np.clip(shade[None, :3] * (shade[None, 3:] + diff[:, None]), dtype(0), dtype(1))
    color = np.zeros((H, W, 3), dtype)
    color[ii, jj] = c
    color_u8 = np.empty((H, W, 3), np.uint8)
    color_u8[...] = np.asarray(background[:3], np.uint8)
    color_u8[ii, jj] = np.floor(dtype(255) * c + dtype(0.5)).astype(np.uint8)
    color[~covered] = np.asarray(background[:3], dtype) / dtype(255)
    return dict(color=color, color_u8=color_u8, depth=np.where(covered, d1, 0).astype(dtype), face_id=fid,
                depth2=d2, count=count)


def ambiguous(r):
    """Pixels whose nearest and second-nearest fragments are closer than 1e-5 of the depth: the winner is not decided there."""
    return (r["face_id"] >= 0) & ((r["depth2"] - r["depth"]) < 1e-5 * r["depth"])


def csr_brute(faces, n_vertices):
    """vertex -> sorted list of the faces that contain it."""
    f = np.asarray(faces).reshape(-1, 3)
    return [sorted({i for i in range(f.shape[0]) if v in f[i]}) for v in range(n_vertices)]
