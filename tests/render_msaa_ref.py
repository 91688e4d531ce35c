"""numpy restatement of the renderer at several sample points per pixel (csrc/render.hip): the truth the
anti-aliasing tests compare against.

It restates render_ref.raster_stage with the sample point as a parameter: a sample (ox, oy), in 1/256 pixel units from the pixel's
top-left corner, is rasterised and shaded exactly as render_ref treats the pixel centre (128, 128), so with that one sample the
arrays are render_ref's bit for bit.  Each sample is restricted to the pixels whose own sample point lies in the face's snapped
bounding box, which is tighter than the kernel's per-pixel box and independent of it.  The resolve is the rounded mean of the
four samples' bytes.  The textured pass is texture_ref's, evaluated at the sample points.  Nothing in the product imports this file.
"""
import numpy as np

import texture_ref as tr
from render_ref import _edge, _top_left, _unit_or_z, face_table

CENTRE = ((128, 128),)
SAMPLES4 = ((96, 32), (224, 96), (32, 160), (160, 224))        # the rotated grid of DESIGN.md 5.27: (x, y) per sample


def _lambert(normals, ids, p, lights, dtype):
    """(1 / pi) sum_k I_k max(0, n . l_k) with n the renormalised interpolated vertex normal: render_ref's lines."""
    nv = np.asarray(normals, np.float32).astype(dtype)[ids]                               # (P, 3 vertices, 3)
    n = _unit_or_z(p[0][:, None] * nv[:, 0] + p[1][:, None] * nv[:, 1] + p[2][:, None] * nv[:, 2])
    lights = np.asarray(lights, np.float32).astype(dtype).reshape(-1, 4)
    diff = np.zeros(n.shape[0], dtype)
    for k in range(lights.shape[0]):
        diff = diff + lights[k, 3] * np.maximum(dtype(0), n[:, 0] * lights[k, 0] + n[:, 1] * lights[k, 1] + n[:, 2] * lights[k, 2])
    return diff * dtype(np.float32(0.318309886183790672))


def raster_samples(screen, normals, faces, height, width, near, far, shade, lights, background, samples=SAMPLES4,
                   dtype=np.float64, fill_rule=True):
    """One frame.  screen / normals (V, 3) fp32 (the vertex stage's outputs), samples ((ox, oy), ...).  Returns a dict of arrays
    with a trailing sample axis S: color (H, W, S, 3) in `dtype` before quantisation, color_u8 (H, W, S, 3), depth (H, W, S) (0 =
    uncovered), face_id (H, W, S) int32 (-1 = uncovered), depth2 (H, W, S) the second-nearest fragment's depth (inf where there
    is none), count (H, W, S) how many faces cover the sample."""
    H, W, S = int(height), int(width), len(samples)
    t = face_table(screen, faces, near)
    X, Y, area = t["X"], t["Y"], t["area"]
    q = dtype(1) / t["d"].astype(dtype)
    out = dict(color=np.zeros((H, W, S, 3), dtype), color_u8=np.empty((H, W, S, 3), np.uint8), depth=np.zeros((H, W, S), dtype),
               face_id=np.full((H, W, S), -1, np.int32), depth2=np.full((H, W, S), np.inf, dtype), count=np.zeros((H, W, S), np.int32))

    def weights(f, px, py):
        e0 = _edge(X[f, 1], Y[f, 1], X[f, 2], Y[f, 2], px, py)
        e1 = _edge(X[f, 2], Y[f, 2], X[f, 0], Y[f, 0], px, py)
        e2 = _edge(X[f, 0], Y[f, 0], X[f, 1], Y[f, 1], px, py)
        A = area[f].astype(dtype)
        w0, w1, w2 = e0.astype(dtype) / A, e1.astype(dtype) / A, e2.astype(dtype) / A
        iz = (w0 * q[f, 0] + w1 * q[f, 1]) + w2 * q[f, 2]
        return (e0, e1, e2), (w0, w1, w2), iz

    shade = np.asarray(shade, np.float32).astype(dtype)
    for k, (ox, oy) in enumerate(samples):
        d1 = np.full((H, W), np.inf, dtype)
        d2 = np.full((H, W), np.inf, dtype)
        fid = np.full((H, W), -1, np.int32)
        count = np.zeros((H, W), np.int32)
        # pixels whose sample point 256 j + ox lies in [xmin, xmax]
        jlo = np.maximum((X.min(1) + 255 - ox) >> 8, 0)
        jhi = np.minimum((X.max(1) - ox) >> 8, W - 1)
        ilo = np.maximum((Y.min(1) + 255 - oy) >> 8, 0)
        ihi = np.minimum((Y.max(1) - oy) >> 8, H - 1)
        live = np.nonzero(t["ok"] & (jlo <= jhi) & (ilo <= ihi))[0]
        for f in live:
            py, px = np.meshgrid(256 * np.arange(ilo[f], ihi[f] + 1, dtype=np.int64) + oy,
                                 256 * np.arange(jlo[f], jhi[f] + 1, dtype=np.int64) + ox, indexing="ij")
            e, _, iz = weights(f, px, py)
            inside = np.ones(px.shape, bool)
            for n, (a, b) in enumerate(((1, 2), (2, 0), (0, 1))):
                keep_zero = bool(_top_left(X[f, a], Y[f, a], X[f, b], Y[f, b])) if fill_rule else True
                inside &= (e[n] > 0) | ((e[n] == 0) & keep_zero)
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
        _, w, iz = weights(f, 256 * jj.astype(np.int64) + ox, 256 * ii.astype(np.int64) + oy)
        p = [w[n] * q[f, n] / iz for n in range(3)]
        diff = _lambert(normals, t["ids"][f], p, lights, dtype)
        c = np.clip(shade[None, :3] * (shade[None, 3:] + diff[:, None]), dtype(0), dtype(1))
        color = np.zeros((H, W, 3), dtype)
        color[ii, jj] = c
        color_u8 = np.empty((H, W, 3), np.uint8)
        color_u8[...] = np.asarray(background[:3], np.uint8)
        color_u8[ii, jj] = np.floor(dtype(255) * c + dtype(0.5)).astype(np.uint8)
        color[~covered] = np.asarray(background[:3], dtype) / dtype(255)
        out["color"][:, :, k], out["color_u8"][:, :, k] = color, color_u8
        out["depth"][:, :, k] = np.where(covered, d1, 0).astype(dtype)
        out["face_id"][:, :, k], out["depth2"][:, :, k], out["count"][:, :, k] = fid, d2, count
    return out


def ambiguous(r):
    """Samples whose nearest and second-nearest fragments are closer than 1e-5 of the depth: the winner is not decided there."""
    return (r["face_id"] >= 0) & ((r["depth2"] - r["depth"]) < 1e-5 * r["depth"])


def resolve(color_u8, covered, background):
    """color_u8 (..., S, 3) uint8 per sample, covered (..., S) bool, background (R, G, B, A) -> (..., 4) uint8: every channel is
    (b0 + ... + b3 + 2) >> 2 over the samples' bytes, a covered sample giving its colour with alpha 255, an uncovered one the
    background's four bytes."""
    color_u8, covered = np.asarray(color_u8), np.asarray(covered, bool)
    assert color_u8.shape[-2] == 4 and covered.shape == color_u8.shape[:-1]
    rgba = np.empty(covered.shape + (4,), np.int64)
    rgba[..., :3] = color_u8
    rgba[..., 3] = 255
    rgba[~covered] = np.asarray(background, np.int64).reshape(4)
    return ((rgba.sum(-2) + 2) >> 2).astype(np.uint8)


def texture_samples(screen, normals, faces, sample_face_id, vt, ft, levels, shade, lights, near, samples=SAMPLES4, dtype=np.float64):
    """One frame of the textured pass at sample positions: texture_ref.texture_stage's formulas with the barycentrics taken at
    sample k of the pixel, and the level of detail from the same per-pixel steps.  sample_face_id (H, W, S) int32 as the raster
    pass leaves it.  Returns covered (H, W, S) (id in [0, F) and a face the set-up keeps), color (H, W, S, 3) before quantisation,
    color_u8 (H, W, S, 3) (zeros where not covered) and lam (H, W, S)."""
    dt = np.dtype(dtype).type
    fid = np.asarray(sample_face_id)
    H, W, S = fid.shape
    L = len(levels)
    Ht, Wt = levels[0].shape[:2]
    faces = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    t = face_table(screen, faces, near)
    X, Y = t["X"], t["Y"]
    covered = (fid >= 0) & (fid < faces.shape[0])
    covered[covered] = t["ok"][fid[covered]]
    ii, jj, kk = np.nonzero(covered)
    f = fid[ii, jj, kk].astype(np.int64)
    off = np.asarray(samples, np.int64)
    px, py = 256 * jj.astype(np.int64) + off[kk, 0], 256 * ii.astype(np.int64) + off[kk, 1]
    A = t["area"][f].astype(dtype)
    q = (dt(1) / t["d"].astype(dtype))[f]
    e = [_edge(X[f, a], Y[f, a], X[f, b], Y[f, b], px, py) for a, b in ((1, 2), (2, 0), (0, 1))]
    w = [e[n].astype(dtype) / A for n in range(3)]
    iz = (w[0] * q[:, 0] + w[1] * q[:, 1]) + w[2] * q[:, 2]
    p = [w[n] * q[:, n] / iz for n in range(3)]
    flip = t["ids"][f, 1] != faces[f, 1]
    k = np.asarray(ft).astype(np.int64).reshape(-1, 3)[f]
    k = np.where(flip[:, None], k[:, [0, 2, 1]], k)
    vt = np.asarray(vt, np.float32)
    inside = (k >= 0) & (k < vt.shape[0])
    uv = np.where(inside[..., None], vt[np.where(inside, k, 0)], np.float32(0)).astype(dtype)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        u = (p[0] * uv[:, 0, 0] + p[1] * uv[:, 1, 0]) + p[2] * uv[:, 2, 0]
        v = (p[0] * uv[:, 0, 1] + p[1] * uv[:, 1, 1]) + p[2] * uv[:, 2, 1]
        a = [-256 * (Y[f, b] - Y[f, a_]) for a_, b in ((1, 2), (2, 0), (0, 1))]
        c = [256 * (X[f, b] - X[f, a_]) for a_, b in ((1, 2), (2, 0), (0, 1))]
        g = [q[:, n] * (a[n].astype(dtype) / A) for n in range(3)]
        h = [q[:, n] * (c[n].astype(dtype) / A) for n in range(3)]
        rho2 = []
        for s in (g, h):
            dD = (s[0] + s[1]) + s[2]
            du = (((s[0] * uv[:, 0, 0] + s[1] * uv[:, 1, 0]) + s[2] * uv[:, 2, 0]) - u * dD) / iz
            dv = (((s[0] * uv[:, 0, 1] + s[1] * uv[:, 1, 1]) + s[2] * uv[:, 2, 1]) - v * dD) / iz
            rho2.append((dt(Wt) * du) * (dt(Wt) * du) + (dt(Ht) * dv) * (dt(Ht) * dv))
        lam = dt(0.5) * np.log2(np.maximum(rho2[0], rho2[1]))
        lam = np.where(np.isfinite(rho2[0]) & np.isfinite(rho2[1]) & np.isfinite(lam), lam, dt(0))
    lam = np.minimum(np.maximum(lam, dt(0)), dt(L - 1)).astype(dtype)
    u, v = tr._finite_or_zero(u).astype(dtype), tr._finite_or_zero(v).astype(dtype)
    T = tr.sample(levels, u, v, lam, dtype)
    diff = _lambert(normals, t["ids"][f], p, lights, dtype)
    shade = np.asarray(shade, np.float32).astype(dtype)
    col = np.clip((T / dt(255)) * (shade[None, 3:] + diff[:, None]), dt(0), dt(1)).astype(dtype)
    out = dict(covered=covered, color=np.zeros((H, W, S, 3), dtype), color_u8=np.zeros((H, W, S, 3), np.uint8), lam=np.zeros((H, W, S), dtype))
    out["color"][ii, jj, kk] = col
    out["color_u8"][ii, jj, kk] = np.floor(dt(255) * col + dt(0.5)).astype(np.uint8)
    out["lam"][ii, jj, kk] = lam
    return out
