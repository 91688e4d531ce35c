"""Per-vertex colours and the error heat map on the MI355X: csrc/render.hip's vertex-colour pass and
csrc/vertex_metrics.hip's error field against the numpy restatements of tests/vertex_color_ref.py.

The shading restatement is fed the GPU's own fp32 screen coordinates, normals and face ids, so no pixel is undecided and every covered
pixel takes part; colours pass under the rule of test_texture_gpu.check_against_reference (uint8 difference <= 1, and the excess over
the half level that rounding costs within render_ref.bound of the float32 yardstick).  At four samples the stored byte is the exact
integer resolve of four quantised samples, so the same rule is applied per sample and carried through the resolve: the byte lies between
the resolves of the least and the greatest byte the rule allows each sample.  The error field is compared byte for byte and bit for bit."""
import functools
import json
import pickle as pkl

import numpy as np
import pytest
import torch

import render_msaa_ref as mr
import render_ref as rr
import vertex_color_ref as vc
from msmd_amd import synth
from test_texture_gpu import DEV, IMAGES, NEAR, T_CENTER, frames, renderer, rots

pytestmark = pytest.mark.gpu
FAR = 3.0
WHITE = (255, 255, 255, 255)
CONSTANT = (200, 120, 40)
KINDS = ("constant", "shared", "per_frame")
CASES = [(m, W, H, B, kind, lit, S) for m in ("a", "b") for W, H, B in IMAGES for kind in KINDS for lit in (True, False) for S in (1, 4)]
case_id = lambda c: f"{c[0]}-{c[1]}x{c[2]}-B{c[3]}-{c[4]}-{'lit' if c[5] else 'unlit'}-S{c[6]}"


@functools.lru_cache(maxsize=None)
def mesh(name):
    if name == "a":
        return synth.latlong_sphere(7, 16, 0.09)
    a = synth.flame_asset()
    return a["v_template"].astype(np.float32), a["f"][:600].astype(np.int32)


@functools.lru_cache(maxsize=None)
def colours(name, kind, B):
    V = mesh(name)[0].shape[0]
    if kind == "constant":
        return np.tile(np.asarray(CONSTANT + (9,), np.uint8), (V, 1))
    return vc.random_colors(f"vertex_color/{name}/{kind}", (V, 4) if kind == "shared" else (B, V, 4))


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


@functools.lru_cache(maxsize=None)
def plain(name, W, H, B, S):
    """The untextured render of a case with its face ids, screen and normals: numpy arrays, shared and never modified."""
    v, f = mesh(name)
    rot = rots(B)
    r = renderer(W, H, samples=S)
    out = r.render_vertices(dev(frames(v, B)), f, t_center=None if rot is None else T_CENTER, rot=rot, return_face_id=True,
                            return_screen=True)
    _, shade, lights = (t.cpu().numpy() for t in r._device_consts(torch.device(DEV)))
    return tuple(t.cpu().numpy() for t in out) + (shade, lights)


@functools.lru_cache(maxsize=None)
def run(name, W, H, B, kind, lit, S):
    v, f = mesh(name)
    rot = rots(B)
    vcol = colours(name, kind, B)
    color, depth, fid = renderer(W, H, samples=S).render_vertices(dev(frames(v, B)), f, t_center=None if rot is None else T_CENTER,
                                                                  rot=rot, return_face_id=True, vertex_colors=vcol, lit=lit)
    torch.cuda.synchronize()
    return color.cpu().numpy(), depth.cpu().numpy(), fid.cpu().numpy()


def reference(name, W, H, B, kind, lit, S, dtype):
    _, f = mesh(name)
    _, _, fid, screen, normals, shade, lights = plain(name, W, H, B, S)
    vcol = colours(name, kind, B)
    out = []
    for b in range(B):
        c = vcol[b] if vcol.ndim == 3 else vcol
        if S == 1:
            out.append(vc.vertex_color_stage(screen[b], normals[b], f, fid[b], c, lit, shade, lights, NEAR, WHITE, dtype))
        else:
            out.append(vc.vertex_color_samples(screen[b], normals[b], f, fid[b], c, lit, shade, lights, NEAR, dtype=dtype))
    return {k: np.stack([o[k] for o in out]) for k in out[0]}


# ---------------------------------------------------------------------------------------------- 1. the shading pass
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_shading_pass_against_the_restatement(case):
    name, W, H, B, kind, lit, S = case
    color, depth, fid = run(*case)
    p_color, p_depth, p_fid = plain(name, W, H, B, S)[:3]
    r64, r32 = reference(*case, np.float64), reference(*case, np.float32)
    covered = r64["covered"]
    assert covered.any() and np.array_equal(covered, fid >= 0)
    # untouched outputs
    assert np.array_equal(depth.view(np.uint32), p_depth.view(np.uint32)) and np.array_equal(fid, p_fid)
    some = covered if S == 1 else covered.any(-1)
    assert (~some).any() and np.array_equal(color[~some], p_color[~some]) and (color[~some] == 255).all()
    lv64, lv32 = 255.0 * r64["color"][covered], 255.0 * r32["color"][covered].astype(np.float64)
    bnd = rr.bound(lv32, lv64)
    if S == 1:
        u8 = r64["color_u8"]
        off = int(np.abs(color[covered].astype(np.int32) - u8[covered].astype(np.int32)).max())
        excess = np.abs(color[covered].astype(np.float64) - lv64) - 0.5
        worst = float((excess / np.maximum(1.0, lv64)).max())
        print(f"{case_id(case)}: {int(covered.sum())} pixels, worst uint8 difference {off}, worst excess over the half level "
              f"{worst / rr.U:.2f} u, bound {bnd / rr.U:.2f} u")
        assert off <= 1 and worst <= bnd
        full = covered
    else:
        want = mr.resolve(r64["color_u8"], covered, WHITE)[..., :3]
        off = int(np.abs(color[some].astype(np.int32) - want[some].astype(np.int32)).max())
        # per sample: the bytes floor(level +- tol + 0.5) the rule allows, tol = bound x max(1, level); then the exact resolve
        level = 255.0 * r64["color"]
        tol = bnd * np.maximum(1.0, level)
        lo = np.clip(np.floor(level - tol + 0.5), 0, 255).astype(np.uint8)
        hi = np.clip(np.floor(level + tol + 0.5), 0, 255).astype(np.uint8)
        least, most = mr.resolve(lo, covered, WHITE)[..., :3], mr.resolve(hi, covered, WHITE)[..., :3]
        inside = (color >= least) & (color <= most)
        loose = int((most[some].astype(np.int32) - least[some].astype(np.int32)).max())
        print(f"{case_id(case)}: {int(some.sum())} pixels with a covered sample, worst uint8 difference {off}, bound {bnd / rr.U:.2f} u, "
              f"{int((~inside[some]).sum())} bytes outside the allowed range (widest range {loose})")
        assert off <= 1 and inside[some].all()
        full = covered.all(-1)
        assert (some & ~full).any()
    if kind == "constant" and not lit:
        assert full.any() and (color[full] == np.asarray(CONSTANT, np.uint8)).all()
    else:
        assert len(np.unique(color[some], axis=0)) > (1 if kind == "constant" else 8)


# ---------------------------------------------------------------------------------------------- 2. orientation
@pytest.mark.parametrize("S", [1, 4])
def test_rewound_faces_give_the_same_image(S):
    v, f = mesh("a")
    half = f.copy()
    half[::2] = half[::2][:, [0, 2, 1]]                       # both windings in one list
    rewound = half[:, [0, 2, 1]]
    vcol = vc.random_colors("vertex_color/orientation", (v.shape[0], 4))
    assert all(len({tuple(vcol[i, :3]) for i in face}) == 3 for face in f[::7])
    from msmd_amd import ops
    r = renderer(64, 64, samples=S)
    verts = dev(v[None])
    # the vertex normals depend on the winding, the pass under test does not: every list is drawn with the normals of `f`
    faces_d, off, ids = r._tables(f, v.shape[0], verts.device)
    view, shade, lights = r._device_consts(verts.device)
    screen, normals = ops.render_vertices(verts, faces_d, off, ids, view, 1.0 / np.tan(r.fov / 2.0), 64, 64)
    vd = dev(vcol)
    for lit in (True, False):
        images = []
        for faces in (f, half, rewound):
            fd = dev(np.ascontiguousarray(faces, np.int32))
            rgba, _, fid = ops.render_raster(screen, normals, fd, shade, lights, 64, 64, NEAR, FAR, 0xffffffff, want_face_id=True, samples=S)
            flat = rgba.clone()
            ops.render_shade_vertex_color(screen, normals, fd, vd, shade, lights, fid, rgba, NEAR, lit=lit, samples=S, background=0xffffffff)
            assert (fid >= 0).any() and not torch.equal(rgba, flat)
            images.append((rgba, fid))
        assert all(torch.equal(images[0][0], x) and torch.equal(images[0][1], y) for x, y in images[1:])
    # through the renderer, unlit: the stored colour does not read the normals
    a, b = (r.render_vertices(verts, faces, vertex_colors=vcol, lit=False)[0] for faces in (half, rewound))
    assert torch.equal(a, b) and torch.equal(a, images[0][0][..., :3])


# ---------------------------------------------------------------------------------------------- 3. determinism
@pytest.mark.parametrize("S", [1, 4])
def test_determinism_and_batch(S):
    v, f = mesh("b")
    W, H, B = 130, 70, 3
    r = renderer(W, H, samples=S)
    verts, rot, tc = dev(frames(v, B)), dev(rots(B)), dev(T_CENTER)
    for kind in ("shared", "per_frame"):
        vcol = dev(colours("b", kind, B))
        call = lambda vv, rr_, cc: r.render_vertices(vv, f, t_center=tc, rot=rr_, return_face_id=True, vertex_colors=cc, lit=False)
        first = [t.clone() for t in call(verts, rot, vcol)]
        again = call(verts, rot, vcol)
        assert all(torch.equal(a, b) for a, b in zip(first, again))
        alone = call(verts[2:3].contiguous(), rot[2:3].contiguous(), vcol[2:3].contiguous() if kind == "per_frame" else vcol)
        assert all(torch.equal(a[2:3], x) for a, x in zip(first, alone))
        assert not torch.equal(first[0][2], first[0][1])


# ---------------------------------------------------------------------------------------------- 4. the error colours
def planted_pair(n, V, half, vmax):
    """pred, gt (n, V, 3) with distances planted at the first and the last vertices: 0, vmax, +inf, NaN (a NaN coordinate and inf -
    inf), the rest random around vmax / 2."""
    g = np.random.default_rng(1000 * V + 10 * n + int(half))
    dt = np.float16 if half else np.float32
    gt = (0.1 * g.standard_normal((n, V, 3))).astype(dt)
    pred = (gt.astype(np.float64) + 0.3 * vmax * g.standard_normal((n, V, 3))).astype(dt)
    plant = [("zero", 0), ("vmax", 1), ("inf", 2), ("nan", 3), ("infinf", 4)]
    for name, k in plant:
        for idx in {k % V, (V - 1 - k) % V}:
            if name == "zero":
                pred[:, idx] = gt[:, idx]
            elif name == "vmax":
                gt[:, idx] = 0
                pred[:, idx] = (0, dt(vmax), 0)
            elif name == "inf":
                pred[:, idx, 1] = np.inf
            elif name == "nan":
                pred[:, idx, 2] = np.nan
            else:
                pred[:, idx, 0] = np.inf
                gt[:, idx, 0] = np.inf
    return pred, gt


@pytest.mark.parametrize("V", [1, 255, 256, 257, 5023])
def test_vertex_error_colors_byte_for_byte(V):
    from msmd_amd import ops
    from msmd_amd.utils.metrics import colormap_table
    lut = colormap_table("jet")
    lut[:, 3] = np.arange(256)                                   # all four bytes of the row travel
    vmax = 0.0078125                                             # 2^-7: exact in fp16, so the planted distance IS vmax
    for half in (False, True):
        for n in (1, 3):
            pred, gt = planted_pair(n, V, half, vmax)
            want = vc.error_colors(pred, gt, vmax, lut, (1, 2, 3, 4))
            got = ops.vertex_error_colors(dev(pred), dev(gt), vmax, dev(lut), (1, 2, 3, 4)).cpu().numpy()
            assert got.shape == (n, V, 4) and got.dtype == np.uint8
            assert np.array_equal(got, want), (V, n, half, int((got != want).any(-1).sum()))
            if V >= 255:
                d = vc.distances(pred, gt)
                assert (d == 0).any() and (d == vmax).any() and np.isposinf(d).any() and np.isnan(d).any()
                assert (want[np.isnan(d)] == (1, 2, 3, 4)).all() and (want[np.isposinf(d)] == lut[255]).all()
                assert (want[d == vmax] == lut[255]).all() and (want[d == 0] == lut[0]).all() and len(np.unique(want[..., 3])) > 50


@pytest.mark.parametrize("N", [1, 255, 257])
def test_colormap_byte_for_byte(N):
    from msmd_amd import ops
    from msmd_amd.utils.metrics import colormap_table
    lut = colormap_table("heat")
    lut[:, 3] = np.arange(256)[::-1]
    vmax = 3.0
    x = np.random.default_rng(N).random(N) * 1.2 * vmax
    for k, val in enumerate((0.0, vmax, np.inf, np.nan, -1.0, -np.inf, vmax / 510.0, np.nextafter(vmax, 0.0))):
        if k < N:
            x[k] = val
    got = ops.colormap(dev(x), vmax, dev(lut)).cpu().numpy()
    assert got.shape == (N, 4) and np.array_equal(got, vc.colormap(x, vmax, lut, (255, 0, 255, 255)))
    if N > 1:
        got2 = ops.colormap(dev(x.reshape(1, N)), vmax, dev(lut), nan_color=(9, 8, 7)).cpu().numpy()
        assert got2.shape == (1, N, 4) and np.array_equal(got2[0], vc.colormap(x, vmax, lut, (9, 8, 7, 255)))


# ---------------------------------------------------------------------------------------------- 5. the error sums
@pytest.mark.parametrize("V", [1, 257])
@pytest.mark.parametrize("half", [False, True])
def test_vertex_error_sums_bit_for_bit(V, half):
    from msmd_amd import ops
    off, n = [0, 1, 6, 8], 8
    g = np.random.default_rng(V + int(half))
    dt = np.float16 if half else np.float32
    pred, gt = g.standard_normal((n, V, 3)).astype(dt), g.standard_normal((n, V, 3)).astype(dt)
    want = vc.error_sums(pred, gt, off)
    o = dev(np.asarray(off, np.int64))

    def sums(p, q, cuts):
        state = torch.zeros(len(off) - 1, V, device=DEV, dtype=torch.float64)
        pd, qd = dev(p), dev(q)
        for a, b in zip(cuts[:-1], cuts[1:]):
            assert ops.vertex_error_sums_(state, pd[a:b], qd[a:b], a, o) is state
        return state.cpu().numpy()

    for chunk in (1, 3, n):
        got = sums(pred, gt, list(range(0, n, chunk)) + [n])
        assert np.array_equal(got.view(np.int64), want.view(np.int64)), (V, half, chunk)
    # a clip's row is the same when the other clips are NaN; and NaN propagates in them
    for k, (a, b) in enumerate(zip(off[:-1], off[1:])):
        p2 = np.full_like(pred, np.nan)
        p2[a:b] = pred[a:b]
        got = sums(p2, gt, [0, 3, n])
        assert np.array_equal(got[k].view(np.int64), want[k].view(np.int64))
        assert all(np.isnan(got[m]).all() for m in range(len(off) - 1) if m != k)
    # the streaming class and the one-call form: the sums over the clips' frame counts
    from msmd_amd.utils import metrics as M
    mean = M.vertex_error_map(dev(pred), dev(gt), off)
    assert mean.is_cuda and mean.dtype == torch.float64 and tuple(mean.shape) == (3, V)
    assert np.array_equal(mean.cpu().numpy().view(np.int64), (want / np.array([[1.0], [5.0], [2.0]])).view(np.int64))
    em = M.VertexErrorMap(off, V, DEV)
    for a, b in ((0, 2), (2, 7), (7, 8)):
        em.update(dev(pred[a:b]), dev(gt[a:b]))
    assert torch.equal(em.result(), mean)
    with pytest.raises(ValueError):
        em.update(dev(pred[:1]), dev(gt[:1]))
    with pytest.raises(ValueError):
        M.VertexErrorMap(off, V, DEV).update(dev(pred[:3]), dev(gt[:3])).result()


# ---------------------------------------------------------------------------------------------- 6. refusals
def test_refusals_come_before_a_launch():
    from msmd_amd import _lib, ops
    from msmd_amd.utils.metrics import colormap_table
    v, f = mesh("a")
    V = v.shape[0]
    lut = dev(colormap_table("jet"))
    p, g = dev(np.zeros((2, V, 3), np.float32)), dev(np.ones((2, V, 3), np.float32))
    x = dev(np.ones(5))
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            ops.vertex_error_colors(p, g, bad, lut)
        with pytest.raises(ValueError):
            ops.colormap(x, bad, lut)
    with pytest.raises(TypeError):
        ops.vertex_error_colors(p, g.half(), 1.0, lut)
    with pytest.raises(TypeError):
        ops.vertex_error_colors(p.double(), g.double(), 1.0, lut)
    with pytest.raises(TypeError):
        ops.vertex_error_colors(p, g, 1.0, lut[:255])
    with pytest.raises(TypeError):
        ops.colormap(x.float(), 1.0, lut)
    with pytest.raises(RuntimeError):
        ops.colormap(x.cpu(), 1.0, lut)
    o = dev(np.asarray([0, 2], np.int64))
    with pytest.raises(TypeError):
        ops.vertex_error_sums_(torch.zeros(1, V, device=DEV, dtype=torch.float64), p, g.half(), 0, o)
    with pytest.raises(TypeError):
        ops.vertex_error_sums_(torch.zeros(1, V + 1, device=DEV, dtype=torch.float64), p, g, 0, o)
    with pytest.raises(ValueError):
        ops.vertex_error_sums_(torch.zeros(1, V, device=DEV, dtype=torch.float64), p, g, -1, o)
    assert tuple(ops.vertex_error_colors(p[:0], g[:0], 1.0, lut).shape) == (0, V, 4)
    # the C ABI says 1 before a launch and leaves its outputs alone
    lib, st = _lib.load(), torch.cuda.current_stream().cuda_stream
    out = torch.full((2, V, 4), 77, device=DEV, dtype=torch.uint8)
    colors = lambda n_, V_, dt, vmax: lib.msmd_vertex_error_colors(p.data_ptr(), g.data_ptr(), lut.data_ptr(), out.data_ptr(), n_, V_, dt,
                                                                   vmax, 0, st)
    for args in ((2, V, ops.F32, 0.0), (2, V, ops.F32, -2.0), (2, V, ops.F32, float("nan")), (2, V, ops.F32, float("inf")),
                 (-1, V, ops.F32, 1.0), (2, 0, ops.F32, 1.0), (2, V, ops.BF16, 1.0)):
        assert colors(*args) == 1, args
    assert colors(0, V, ops.F32, 1.0) == 0
    assert lib.msmd_vertex_error_colors(p.data_ptr(), g.data_ptr(), None, out.data_ptr(), 2, V, ops.F32, 1.0, 0, st) == 1
    assert lib.msmd_colormap_f64(x.data_ptr(), lut.data_ptr(), out.data_ptr(), 5, 0.0, 0, st) == 1
    assert lib.msmd_colormap_f64(x.data_ptr(), lut.data_ptr(), out.data_ptr(), -1, 1.0, 0, st) == 1
    assert lib.msmd_colormap_f64(x.data_ptr(), lut.data_ptr(), out.data_ptr(), 0, 1.0, 0, st) == 0
    state = torch.full((1, V), 5.0, device=DEV, dtype=torch.float64)
    sums = lambda n_, V_, C_, f0, dt: lib.msmd_vertex_error_sums(p.data_ptr(), g.data_ptr(), f0, n_, o.data_ptr(), C_, state.data_ptr(), V_, dt, st)
    for args in ((-1, V, 1, 0, ops.F32), (2, 0, 1, 0, ops.F32), (2, V, 0, 0, ops.F32), (2, V, 1, -1, ops.F32), (2, V, 1, 0, ops.BF16)):
        assert sums(*args) == 1, args
    assert sums(0, V, 1, 0, ops.F32) == 0
    torch.cuda.synchronize()
    assert (out == 77).all() and (state == 5.0).all()
    # the renderer and its op
    r = renderer(37, 53)
    r4 = renderer(37, 53, samples=4)
    dv = dev(v[None])
    vcol = vc.random_colors("vertex_color/refusals", (V, 4))
    from test_texture_gpu import mesh as tex_mesh, texture
    _, _, vt, ft = tex_mesh("a")
    with pytest.raises(TypeError):
        r.render_vertices(dv, f, vertex_colors=vcol, tex_img=texture("8x8"), tex_uv={"vt": vt, "ft": ft})
    for bad, err in ((np.zeros((V + 1, 4), np.uint8), ValueError), (vcol[:, :2], ValueError), (np.zeros((2, V, 4), np.uint8), ValueError),
                     (vcol.astype(np.float32), TypeError), (vcol[0], ValueError)):
        with pytest.raises(err, match=rf"\({V}, 3 \| 4\)"):
            r.render_vertices(dv, f, vertex_colors=bad)
    faces_d, off, ids = r._tables(f, V, dv.device)
    view, shade, lights = r._device_consts(dv.device)
    screen, normals = ops.render_vertices(dv, faces_d, off, ids, view, 1.0 / np.tan(r.fov / 2.0), 53, 37)
    rgba, _, fid = ops.render_raster(screen, normals, faces_d, shade, lights, 53, 37, NEAR, FAR, 0xffffffff, want_face_id=True)
    rgba4, _, fid4 = ops.render_raster(screen, normals, faces_d, shade, lights, 53, 37, NEAR, FAR, 0xffffffff, want_face_id=True, samples=4)
    vd = dev(vcol)
    good = (screen, normals, faces_d, vd, shade, lights, fid, rgba, NEAR)
    before = rgba.clone()
    with pytest.raises(ValueError):
        ops.render_shade_vertex_color(*good, samples=2)
    with pytest.raises(ValueError):
        ops.render_shade_vertex_color(screen, normals, faces_d, vd, shade, lights, fid4, rgba4, NEAR, samples=4)      # no background
    with pytest.raises(TypeError):
        ops.render_shade_vertex_color(*good, samples=4, background=0xffffffff)                                        # one-sample ids
    for k, bad in ((3, dev(np.zeros((V + 1, 4), np.uint8))), (3, vd[:, :3]), (3, vd.cpu()), (3, vd.int()), (3, dev(np.zeros((2, V, 4), np.uint8))),
                   (6, fid.long()), (7, rgba[..., :3]), (4, shade[:3]), (0, screen[:, :-1].contiguous())):
        args = list(good)
        args[k] = bad
        with pytest.raises(TypeError):
            ops.render_shade_vertex_color(*args)
    call = lambda samples, near=NEAR, B_=1: lib.msmd_render_shade_vertex_color(
        screen.data_ptr(), normals.data_ptr(), faces_d.data_ptr(), vd.data_ptr(), 0, 1, shade.data_ptr(), lights.data_ptr(), lights.shape[0],
        fid.data_ptr(), rgba.data_ptr(), B_, V, faces_d.shape[0], 53, 37, near, 0xffffffff, samples, st)
    assert call(2) == 1 and call(0) == 1 and call(3) == 1 and call(1, 0.0) == 1 and call(1, NEAR, 0) == 1
    torch.cuda.synchronize()
    assert torch.equal(rgba, before)
    assert ops.render_shade_vertex_color(*good) is None and not torch.equal(rgba, before)


# ---------------------------------------------------------------------------------------------- 7. end to end
def test_render_comparison_panels_and_legend():
    from msmd_amd import ops
    from msmd_amd.utils import metrics as M
    v, f = mesh("a")
    n, W, H = 5, 64, 48
    g = np.random.default_rng(3)
    gt = dev(frames(v, n))
    pred = gt + dev((0.004 * g.standard_normal((n,) + v.shape)).astype(np.float32))
    vmax = 0.01
    r = renderer(W, H)
    out = M.render_comparison(pred, gt, f, r, vmax, table="heat")
    assert out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == (n, H, 3 * W, 3)
    lut = M.colormap_table("heat")
    bar = max(4, W // 32)
    assert torch.equal(out[:, :, :W], r.render_vertices(gt, f)[0]) and torch.equal(out[:, :, W:2 * W], r.render_vertices(pred, f)[0])
    err = r.render_vertices(pred, f, vertex_colors=ops.vertex_error_colors(pred, gt, vmax, dev(lut)), lit=False)[0]
    assert torch.equal(out[:, :, 2 * W:3 * W - bar], err[:, :, :W - bar])
    rows = lut[255 - (np.arange(H) * 256) // H, :3]
    legend = out[:, :, 3 * W - bar:].cpu().numpy()
    assert legend.shape == (n, H, bar, 3) and (legend == rows[None, :, None, :]).all()
    assert tuple(rows[0]) == tuple(lut[255, :3]) and tuple(rows[-1]) == tuple(lut[255 - ((H - 1) * 256) // H, :3])
    # the heat map is not the plain render, and it shows more than one colour of the table
    assert not torch.equal(err, r.render_vertices(pred, f)[0]) and len(np.unique(err.cpu().numpy().reshape(-1, 3), axis=0)) > 16
    # panels and legend are arguments; a user table is taken
    two = M.render_comparison(pred, gt, f, r, vmax, table=lut[:, :3].copy(), panels=("error", "gt"), legend=False)
    assert tuple(two.shape) == (n, H, 2 * W, 3) and torch.equal(two[:, :, :W], err) and torch.equal(two[:, :, W:], out[:, :, :W])
    with pytest.raises(ValueError):
        M.render_comparison(pred, gt, f, r, vmax, panels=("gt", "depth"))
    with pytest.raises(ValueError):
        M.render_comparison(pred, gt, f, r, 0.0)


def test_command_line_writes_the_video_the_still_and_the_scales(tmp_path):
    from msmd_amd.utils import media, metrics as M
    asset = synth.flame_asset()
    with open(tmp_path / "flame.pkl", "wb") as fh:
        pkl.dump({k: v for k, v in asset.items() if k != "lmk"}, fh)
    np.save(tmp_path / "lmk.npy", np.array(asset["lmk"], dtype=object), allow_pickle=True)
    g = np.random.default_rng(5)
    T = 7
    gt = np.concatenate([0.8 * g.standard_normal((T, 50)), 0.2 * g.standard_normal((T, 3))], 1).astype(np.float32)
    pred = gt + (0.05 * g.standard_normal((T, 53))).astype(np.float32)
    for name, val in (("pe", pred[:, :50]), ("pr", pred[:, 50:]), ("ge", gt[:, :50]), ("gr", gt[:, 50:])):
        with open(tmp_path / f"{name}.pkl", "wb") as fh:
            pkl.dump(val, fh)
    np.savez(tmp_path / "masks.npz", lips=np.arange(1000, 1200), upper=np.arange(3000, 4000, 3))
    base = ["--pred_exp", str(tmp_path / "pe.pkl"), "--pred_rot", str(tmp_path / "pr.pkl"), "--gt_exp", str(tmp_path / "ge.pkl"),
            "--gt_rot", str(tmp_path / "gr.pkl"), "--regions", str(tmp_path / "masks.npz"), "--flame_model_path", str(tmp_path / "flame.pkl"),
            "--flame_lmk_embedding_path", str(tmp_path / "lmk.npy"), "--chunk", "3"]
    plain = M.main(base + ["--out", str(tmp_path / "plain.json")])
    res = M.main(base + ["--out", str(tmp_path / "m.json"), "--comparison_video", str(tmp_path / "c.avi"), "--error_map",
                         str(tmp_path / "e.jpg"), "--render_size", "64", "--colormap", "heat"])
    with open(tmp_path / "m.json") as fh:
        written = json.load(fh)
    assert written["all"] == plain["all"] and written["clips"] == plain["clips"]        # the metrics do not know they were drawn
    assert written["error_max_video"] == plain["all"]["max_ve"] and 0 < written["error_max_map"] <= written["error_max_video"]
    assert written["colormap"] == "heat" and res["error_max_map"] == written["error_max_map"]
    clip = media.read_avi(str(tmp_path / "c.avi"))
    assert len(clip.frames) == T and tuple(clip.size) == (3 * 64, 64) and clip.fps == 25 and clip.audio is None
    still = media.decode_jpeg([(tmp_path / "e.jpg").read_bytes()])
    assert tuple(still.shape) == (1, 64, 64, 3)
    # a given scale is one pass: the same frames when it is the data's own maximum
    one = M.main(base + ["--out", str(tmp_path / "one.json"), "--comparison_video", str(tmp_path / "one.avi"), "--render_size", "64",
                         "--colormap", "heat", "--error_max", repr(written["error_max_video"])])
    assert one["error_max_video"] == written["error_max_video"] and "error_max_map" not in one
    again = media.read_avi(str(tmp_path / "one.avi"))
    assert len(again.frames) == T and all(bytes(again.jpeg(k)) == bytes(clip.jpeg(k)) for k in range(T))
