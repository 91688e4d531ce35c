"""numpy restatements of the error field, its colours and the vertex-colour shading pass (csrc/vertex_metrics.hip, csrc/render.hip;
DESIGN.md 5.30): the truth the vertex-colour tests compare against.

The error field is float64, operation by operation, from the exact float64 images of the stored values: the kernels must give the
same bytes (colours) and the same bits (sums).  The shading pass runs on fp32 screen coordinates and normals and an int32 face-id
map (the raster stage's outputs) in the dtype asked for: float64 is the truth, float32 (the same operations in the same order) the
yardstick the bounds are taken from.  The face set-up is render_ref's, the sample positions and the resolve render_msaa_ref's.
Nothing in the product imports this file.
"""
import numpy as np

import render_msaa_ref as mr
import render_ref as rr

NAN_COLOR = (255, 0, 255, 255)


# ------------------------------------------------------------------------------------------------ the error field
def distances(pred, gt):
    """(n, V, 3) fp32 or fp16 -> d (n, V) float64 = sqrt((dx dx + dy dy) + dz dz), every operation rounded on its own."""
    p, g = np.asarray(pred).astype(np.float64), np.asarray(gt).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy, dz = p[..., 0] - g[..., 0], p[..., 1] - g[..., 1], p[..., 2] - g[..., 2]
        return np.sqrt((dx * dx + dy * dy) + dz * dz)


def colormap(x, vmax, lut, nan_color=NAN_COLOR):
    """x float64 of any shape -> x.shape + (4,) uint8: t = x / vmax; NaN -> nan_color; t >= 1 -> row 255; t <= 0 -> row 0; else row
    floor(t * 255 + 0.5)."""
    x, lut = np.asarray(x, np.float64), np.asarray(lut, np.uint8)
    assert lut.shape == (256, 4) and np.isfinite(vmax) and vmax > 0
    with np.errstate(invalid="ignore", over="ignore"):
        t = x / np.float64(vmax)
        mid = np.floor(np.where((t > 0) & (t < 1), t, 0.0) * 255.0 + 0.5).astype(np.int64)
    idx = np.where(t >= 1.0, 255, np.where(t > 0.0, mid, 0))
    out = lut[idx]
    out[np.isnan(t)] = np.asarray(nan_color, np.uint8)
    return out


def error_colors(pred, gt, vmax, lut, nan_color=NAN_COLOR):
    """-> (n, V, 4) uint8: the colour rule at the per-vertex distance."""
    return colormap(distances(pred, gt), vmax, lut, nan_color)


def error_sums(pred, gt, clip_offsets, cuts=None):
    """-> (n_clips, V) float64: per clip and vertex the distances of the clip's frames added in frame order, one addition at a time.
    `cuts` (chunk boundaries from 0 to n) walks the sequence chunk by chunk as the kernel does, the state carried between chunks."""
    d = distances(pred, gt)
    n = d.shape[0]
    off = [int(o) for o in clip_offsets]
    cuts = [0, n] if cuts is None else list(cuts)
    state = np.zeros((len(off) - 1, d.shape[1]), np.float64)
    for a, b in zip(cuts[:-1], cuts[1:]):
        for k, (c0, c1) in enumerate(zip(off[:-1], off[1:])):
            for f in range(max(a, c0), min(b, c1)):
                state[k] = state[k] + d[f]
    return state


# ------------------------------------------------------------------------------------------------ the shading pass
def _shade_points(t, f, px, py, normals, vcol, lit, shade, lights, dtype):
    """Colour before quantisation, (P, 3) in `dtype`, of faces f (P,) at the points (px, py) in 1 / 256 pixel units."""
    dt = np.dtype(dtype).type
    X, Y = t["X"], t["Y"]
    A = t["area"][f].astype(dtype)
    q = (dt(1) / t["d"].astype(dtype))[f]
    e = [rr._edge(X[f, a], Y[f, a], X[f, b], Y[f, b], px, py) for a, b in ((1, 2), (2, 0), (0, 1))]
    w = [e[k].astype(dtype) / A for k in range(3)]
    iz = (w[0] * q[:, 0] + w[1] * q[:, 1]) + w[2] * q[:, 2]
    p = [w[k] * q[:, k] / iz for k in range(3)]
    c = np.asarray(vcol, np.uint8)[t["ids"][f]][..., :3].astype(dtype)             # (P, 3 corners, 3 channels), oriented order
    C = (p[0][:, None] * c[:, 0] + p[1][:, None] * c[:, 1]) + p[2][:, None] * c[:, 2]
    col = C / dt(255)
    if lit:
        diff = mr._lambert(normals, t["ids"][f], p, lights, dtype)
        shade = np.asarray(shade, np.float32).astype(dtype)
        col = col * (shade[None, 3:] + diff[:, None])
    return np.clip(col, dt(0), dt(1)).astype(dtype)


def vertex_color_stage(screen, normals, faces, face_id, vcol, lit, shade, lights, near, background, dtype=np.float64):
    """One frame at one sample per pixel.  screen / normals (V, 3) fp32 and face_id (H, W) int32 as the raster stage leaves them;
    vcol (V, 3 | 4) uint8.  Returns color (H, W, 3) before quantisation, color_u8 and covered; the background outside the mesh."""
    dt = np.dtype(dtype).type
    fid = np.asarray(face_id)
    faces = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    t = rr.face_table(screen, faces, near)
    covered = (fid >= 0) & (fid < faces.shape[0])
    covered[covered] = t["ok"][fid[covered]]
    ii, jj = np.nonzero(covered)
    f = fid[ii, jj].astype(np.int64)
    col = _shade_points(t, f, 256 * jj.astype(np.int64) + 128, 256 * ii.astype(np.int64) + 128, normals, vcol, lit, shade, lights, dtype)
    out = dict(covered=covered, color=np.empty(fid.shape + (3,), dtype), color_u8=np.empty(fid.shape + (3,), np.uint8))
    out["color"][...] = np.asarray(background[:3], dtype) / dt(255)
    out["color"][ii, jj] = col
    out["color_u8"][...] = np.asarray(background[:3], np.uint8)
    out["color_u8"][ii, jj] = np.floor(dt(255) * col + dt(0.5)).astype(np.uint8)
    return out


def vertex_color_samples(screen, normals, faces, sample_face_id, vcol, lit, shade, lights, near, samples=mr.SAMPLES4, dtype=np.float64):
    """One frame at several samples per pixel: the stage's formulas at sample k of the pixel.  sample_face_id (H, W, S) int32.  Returns
    covered (H, W, S), color (H, W, S, 3) before quantisation and color_u8 (zeros where not covered); render_msaa_ref.resolve makes the
    pixel."""
    dt = np.dtype(dtype).type
    fid = np.asarray(sample_face_id)
    faces = np.asarray(faces).astype(np.int64).reshape(-1, 3)
    t = rr.face_table(screen, faces, near)
    covered = (fid >= 0) & (fid < faces.shape[0])
    covered[covered] = t["ok"][fid[covered]]
    ii, jj, kk = np.nonzero(covered)
    f = fid[ii, jj, kk].astype(np.int64)
    off = np.asarray(samples, np.int64)
    col = _shade_points(t, f, 256 * jj.astype(np.int64) + off[kk, 0], 256 * ii.astype(np.int64) + off[kk, 1], normals, vcol, lit, shade,
                        lights, dtype)
    out = dict(covered=covered, color=np.zeros(fid.shape + (3,), dtype), color_u8=np.zeros(fid.shape + (3,), np.uint8))
    out["color"][ii, jj, kk] = col
    out["color_u8"][ii, jj, kk] = np.floor(dt(255) * col + dt(0.5)).astype(np.uint8)
    return out


def random_colors(name, shape):
    """Seeded uniform bytes of the given shape (…, 4)."""
    from msmd_amd import synth
    return np.floor(synth.uniform01(name, int(np.prod(shape))) * np.float32(256)).astype(np.uint8).reshape(shape)
