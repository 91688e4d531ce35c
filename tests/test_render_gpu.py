"""The HIP mesh renderer (csrc/render.hip, utils/renderer.MeshRenderer) against the numpy truth of tests/render_ref.py.

Stage by stage: the vertex stage against float64; the raster stage against the reference's raster stage fed with the GPU's own
fp32 screen coordinates and normals, so coverage is compared exactly.  Bounds have the form max(16 u, 4 x yardstick), u = 2^-24,
the yardstick being the same restatement run in float32 numpy on the same inputs."""
import functools

import numpy as np
import pytest
import torch

import render_ref as rr
from msmd_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NEAR, FAR = 0.01, 3.0


@functools.lru_cache(maxsize=None)
def mesh(name):
    if name == "a":            # small closed sphere
        return synth.latlong_sphere(7, 16, 0.09)
    if name == "b":            # large overlapping triangles, heavy overdraw
        a = synth.flame_asset()
        return a["v_template"].astype(np.float32), a["f"][:600].astype(np.int32)
    if name == "c":            # sub-pixel triangles at 128 x 128: many cover no pixel centre
        return synth.latlong_sphere(49, 100, 0.09)
    raise KeyError(name)


def rots(B):
    return (0.5 * synth.normalish("render/rot", (3, 3)))[:B].astype(np.float32) if B > 1 else None


# (mesh, W, H, B): B > 1 turns every frame by its own axis-angle about T_CENTER
CASES = [("a", 64, 64, 1), ("a", 37, 53, 3), ("a", 130, 70, 1), ("b", 64, 64, 1), ("b", 130, 70, 3), ("b", 128, 128, 1),
         ("c", 128, 128, 1), ("c", 37, 53, 1)]
T_CENTER = np.array([0.01, -0.02, 0.005], np.float32)


def renderer(W, H, **kw):
    from msmd_amd.utils.renderer import MeshRenderer
    return MeshRenderer((W, H), **kw)


@functools.lru_cache(maxsize=None)
def run(name, W, H, B):
    """One GPU render of a case and its references, computed once and shared (nothing below modifies them)."""
    v, f = mesh(name)
    r = renderer(W, H)
    verts = np.stack([v * np.float32(1.0 + 0.02 * b) for b in range(B)])
    rot = rots(B)
    color, depth, fid, screen, normals = r.render_vertices(
        torch.from_numpy(verts).to(DEV), torch.from_numpy(f).to(DEV), t_center=None if rot is None else T_CENTER,
        rot=rot, return_face_id=True, return_screen=True)
    torch.cuda.synchronize()
    view, shade, lights = (t.cpu().numpy() for t in r._device_consts(torch.device(DEV)))
    focal = np.float32(1.0 / np.tan(r.fov / 2.0))
    g = dict(color=color.cpu().numpy(), depth=depth.cpu().numpy(), face_id=fid.cpu().numpy(), screen=screen.cpu().numpy(),
             normals=normals.cpu().numpy())
    vs = {dt: rr.vertex_stage(verts, f, view, focal, H, W, T_CENTER, rot, dt) for dt in (np.float64, np.float32)}
    rs = {dt: [rr.raster_stage(g["screen"][b], g["normals"][b], f, H, W, NEAR, FAR, shade, lights, r.bg_color, dt)
               for b in range(B)] for dt in (np.float64, np.float32)}
    return g, vs, rs


def stacked(rs, key):
    return np.stack([x[key] for x in rs])


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-{c[1]}x{c[2]}-B{c[3]}")
def test_vertex_stage(case):
    g, vs, _ = run(*case)
    for k, key in enumerate(("screen", "normals")):
        s64, s32 = vs[np.float64][k], vs[np.float32][k]
        parts = (("xy", slice(0, 2)), ("depth", slice(2, 3))) if key == "screen" else (("n", slice(0, 3)),)
        for tag, sl in parts:
            err = float(rr.rel_err(g[key][..., sl], s64[..., sl]).max())
            bnd = rr.bound(s32[..., sl], s64[..., sl])
            print(f"{case} {key}.{tag}: max err {err / rr.U:.2f} u, yardstick {float(rr.rel_err(s32[..., sl], s64[..., sl]).max()) / rr.U:.2f} u")
            assert err <= bnd, (key, tag, err / rr.U, bnd / rr.U)


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}-{c[1]}x{c[2]}-B{c[3]}")
def test_coverage_face_id_depth_colour(case):
    g, _, rs = run(*case)
    r64, r32 = rs[np.float64], rs[np.float32]
    fid64 = stacked(r64, "face_id")
    covered = fid64 >= 0
    assert covered.any()
    # 2. coverage is exact
    assert torch.equal(torch.from_numpy(g["face_id"] >= 0), torch.from_numpy(covered))
    # 3. the winning face, outside the pixels the reference cannot decide
    amb = np.stack([rr.ambiguous(x) for x in r64])
    print(f"{case}: {int(covered.sum())} covered pixels, {int(amb.sum())} ambiguous")
    assert amb.sum() <= 0.005 * covered.sum()
    sure = covered & ~amb
    assert np.array_equal(g["face_id"][sure], fid64[sure])
    # 4. depth and colour where the winner is decided (and the float32 restatement agrees on it)
    sure &= stacked(r32, "face_id") == fid64
    d64, d32 = stacked(r64, "depth"), stacked(r32, "depth")
    err = float(rr.rel_err(g["depth"][sure], d64[sure]).max())
    bnd = rr.bound(d32[sure], d64[sure])
    print(f"{case} depth: max err {err / rr.U:.2f} u, bound {bnd / rr.U:.2f} u")
    assert err <= bnd
    u8 = stacked(r64, "color_u8")
    assert np.abs(g["color"][sure].astype(np.int32) - u8[sure].astype(np.int32)).max() <= 1
    # before quantisation, in units of one level (1 / 255): the kernel's unquantised colour is not stored, so its uint8 is
    # held to the reference's unquantised level within the half level rounding costs plus the bound
    lv64, lv32 = 255.0 * stacked(r64, "color")[sure], 255.0 * stacked(r32, "color")[sure].astype(np.float64)
    bnd = rr.bound(lv32, lv64)
    excess = np.abs(g["color"][sure].astype(np.float64) - lv64) - 0.5
    worst = float((excess / np.maximum(1.0, lv64)).max())
    print(f"{case} colour: worst excess over the half level {worst / rr.U:.2f} u, bound {bnd / rr.U:.2f} u")
    assert worst <= bnd
    # background: its colour exactly, depth exactly 0, face id -1
    assert (g["color"][~covered] == 255).all() and (g["depth"][~covered] == 0.0).all() and (g["face_id"][~covered] == -1).all()


def test_degenerate_inputs():
    r = renderer(64, 64)
    v = np.array([[-0.05, -0.05, 0], [0.05, -0.05, 0], [0, 0.05, 0],      # 0-2: a visible triangle
                  [0, 0, 0.995], [0.001, 0, 0.995], [0, 0.001, 0.995],    # 3-5: nearer than `near` (depth 0.005)
                  [5, 5, 0], [5.1, 5, 0], [5, 5.1, 0]], np.float32)       # 6-8: far off-screen
    full = np.array([[0, 1, 2], [0, 0, 1], [3, 4, 5], [6, 7, 8]], np.int32)
    want = None
    for faces in (full[:1], full):                    # F = 1, then with the faces that must draw nothing
        c, d, fid = r.render_vertices(torch.from_numpy(v[None]).to(DEV), faces, return_face_id=True)
        fid = fid.cpu().numpy()
        assert set(np.unique(fid)) == {-1, 0}
        want = (c.clone(), d.clone()) if want is None else want
        assert torch.equal(c, want[0]) and torch.equal(d, want[1])
    c, d, fid = r.render_vertices(torch.from_numpy(v[None]).to(DEV), full[1:], return_face_id=True)   # nothing visible
    assert (fid == -1).all() and (d == 0).all() and (c == 255).all()
    cb, _ = renderer(64, 64, black_bg=True).render_vertices(torch.from_numpy(v[None]).to(DEV), full[3:])
    assert (cb == 0).all()


def test_determinism_graph_and_batch():
    v, f = mesh("b")
    W, H, B = 130, 70, 3
    r = renderer(W, H)
    verts = torch.from_numpy(np.stack([v * np.float32(1.0 + 0.02 * b) for b in range(B)])).to(DEV)
    faces = torch.from_numpy(f).to(DEV)
    rot = torch.from_numpy(rots(B)).to(DEV)
    tc = torch.from_numpy(T_CENTER).to(DEV)
    call = lambda vv, rr_: r.render_vertices(vv, faces, t_center=tc, rot=rr_, return_face_id=True)
    first = [t.clone() for t in call(verts, rot)]
    again = call(verts, rot)
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    for b in range(B):                                  # a frame of the batch equals that frame rendered alone
        alone = call(verts[b:b + 1].contiguous(), rot[b:b + 1].contiguous())
        assert all(torch.equal(a[b:b + 1], x) for a, x in zip(first, alone))
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call(verts, rot)
    torch.cuda.current_stream().wait_stream(side)
    with torch.cuda.graph(graph):
        captured = call(verts, rot)
    for t in captured:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(first, captured))


def test_surface():
    from msmd_amd import ops
    v, f = mesh("a")
    r = renderer(37, 53)
    mesh_obj = type("Mesh", (), {"v": v.astype(np.float64), "f": f.astype(np.uint32)})()
    rot = np.array([0.1, 0.3, -0.2])
    color, depth = r.render_mesh(mesh_obj, T_CENTER, rot)
    assert isinstance(color, np.ndarray) and color.dtype == np.uint8 and color.shape == (53, 37, 3)
    assert isinstance(depth, np.ndarray) and depth.dtype == np.float32 and depth.shape == (53, 37)
    dv = torch.from_numpy(v[None]).to(DEV)
    c2, d2 = r.render_vertices(dv, f, t_center=T_CENTER, rot=rot)
    assert c2.is_cuda and c2.dtype == torch.uint8 and tuple(c2.shape) == (1, 53, 37, 3) and d2.dtype == torch.float32
    assert np.array_equal(c2[0].cpu().numpy(), color) and np.array_equal(d2[0].cpu().numpy(), depth)
    assert (depth > 0).any() and (depth == 0).any()
    with pytest.raises(NotImplementedError):
        r.render_mesh(mesh_obj, T_CENTER, tex_img=np.zeros((4, 4, 3), np.uint8))
    # fp16 vertices (FLAME.vertex_dtype = float16) render as their fp32 values
    ch, dh = r.render_vertices(dv.half(), f)
    cf, df = r.render_vertices(dv.half().float(), f)
    assert torch.equal(ch, cf) and torch.equal(dh, df) and (dh > 0).any()
    # the tables are cached per faces tensor
    ft = torch.from_numpy(f).to(DEV)
    r.render_vertices(dv, ft)
    n = len(r._csr)
    r.render_vertices(dv, ft)
    assert len(r._csr) == n
    # ops take contiguous fp32 / int32 CUDA tensors only
    faces_d, off, ids = r._tables(ft, v.shape[0], dv.device)
    view, shade, lights = r._device_consts(dv.device)
    good = (dv, faces_d, off, ids, view, 7.0, 53, 37)
    screen, normals = ops.render_vertices(*good)
    strided = torch.zeros(1, v.shape[0], 6, device=DEV)[..., ::2]
    for k, bad in ((0, dv.cpu()), (0, strided),
                   (0, dv.double()), (1, faces_d.long()), (1, faces_d.t()), (4, view.cpu())):
        args = list(good)
        args[k] = bad
        with pytest.raises(TypeError):
            ops.render_vertices(*args)
    good = (screen, normals, faces_d, shade, lights, 53, 37, NEAR, FAR, 0xffffffff)
    for k, bad in ((0, screen.cpu()), (1, normals[:, ::2]), (2, faces_d.long()), (4, lights.t())):
        args = list(good)
        args[k] = bad
        with pytest.raises(TypeError):
            ops.render_raster(*args)


def test_argument_spec():
    """ops._arg, the one check between a caller of the data-prep and media wrappers and a kernel that indexes raw pointers."""
    from msmd_amd import ops
    f32, i32 = torch.float32, torch.int32
    z = lambda *shape, dtype=f32: torch.zeros(*shape, dtype=dtype, device=DEV)
    d = {}
    ops._arg("verts", z(2, 5, 3), f32, "B V 3", d)
    ops._arg("faces", z(7, 3, dtype=i32), i32, "F 3", d)
    assert d == {"B": 2, "V": 5, "F": 7}
    ops._arg("csr_offsets", z(6, dtype=i32), i32, (d["V"] + 1,))
    # a name bound by one argument and violated by a later one: the later argument, the bound size and the offending one
    with pytest.raises(TypeError, match=r"normals must have shape \(2, 5, 3\), got \(2, 4, 3\)"):
        ops._arg("normals", z(2, 4, 3), f32, "B V 3", d)
    with pytest.raises(TypeError, match=r"ft must have shape \(7, 3\), got \(6, 3\)"):
        ops._arg("ft", z(6, 3, dtype=i32), i32, "F 3", d)
    assert d == {"B": 2, "V": 5, "F": 7}                                   # a refused argument binds nothing
    with pytest.raises(TypeError, match=r"lights must have shape \(L, 4\), got \(4,\)"):
        ops._arg("lights", z(4), f32, "L 4", d)
    with pytest.raises(TypeError, match=r"view must have shape \(3, 4\), got \(4, 3\)"):
        ops._arg("view", z(4, 3), f32, "3 4")
    with pytest.raises(TypeError, match=r"m must have shape \(n, n\), got \(2, 3\)"):
        ops._arg("m", z(2, 3), f32, "n n")
    # a set entry
    for c in (3, 4):
        ops._arg("img", z(8, 9, c, dtype=torch.uint8), torch.uint8, ("Ht", "Wt", (3, 4)))
    with pytest.raises(TypeError, match=r"img must have shape \(Ht, Wt, 3 \| 4\), got \(8, 9, 2\)"):
        ops._arg("img", z(8, 9, 2, dtype=torch.uint8), torch.uint8, ("Ht", "Wt", (3, 4)))
    # "+": at least one
    ops._arg("vt", z(1, 2), f32, "Nt+ 2")
    ops._arg("faces", z(0, 3, dtype=i32), i32, "F 3")
    with pytest.raises(TypeError, match=r"vt must have shape \(Nt, 2\), got \(0, 2\)"):
        ops._arg("vt", z(0, 2), f32, "Nt+ 2")
    # None passes only where it may; a tensor is contiguous, on the device and of the stated dtype
    ops._arg("rot", None, f32, "B 3", d, optional=True)
    for bad in (None, np.zeros((2, 3), np.float32), z(2, 3).cpu(), z(2, 3).double(), z(2, 3, dtype=i32), z(3, 2).t(), z(2, 6)[:, ::2]):
        with pytest.raises(TypeError, match="rot must be a contiguous torch.float32 CUDA tensor"):
            ops._arg("rot", bad, f32, "B 3", d)
    # the Savitzky-Golay table of the smoothing wrappers goes through the same check
    assert ops._savgol_window(5, ("table", z(25, dtype=torch.float64))) == 5
    with pytest.raises(TypeError, match=r"table must have shape \(25,\), got \(24,\)"):
        ops._savgol_window(5, ("table", z(24, dtype=torch.float64)))
    with pytest.raises(TypeError, match="table must be a contiguous torch.float64"):
        ops._savgol_window(5, ("table", z(25)))
    with pytest.raises(TypeError, match="table must be a contiguous torch.float64"):
        ops._savgol_window(5, ("table", None))


def test_render_coeffs_equals_the_chain():
    from types import SimpleNamespace
    from msmd_amd.inference import render_coeffs
    from msmd_amd.utils.common import coef_dict_to_vertices, get_coef_dict
    from msmd_amd.utils.flame import FLAME, FLAMEConfig
    cfg = SimpleNamespace(**vars(FLAMEConfig))
    cfg.asset = synth.flame_asset()
    flame = FLAME(cfg).to(DEV)
    T = 3
    coef = torch.from_numpy(0.3 * synth.normalish("render/coef", (T, 54))).float().to(DEV)
    shape = torch.from_numpy(0.3 * synth.normalish("render/shape", (1, 100))).float().to(DEV)
    r = renderer(64, 64)
    frames = render_coeffs(coef, shape, flame, None, r, chunk=2)          # two chunks
    assert frames.dtype == torch.uint8 and tuple(frames.shape) == (T, 64, 64, 3) and frames.is_cuda
    verts = coef_dict_to_vertices(get_coef_dict(coef, shape.expand(T, -1), None, with_global_pose=True), flame)
    want, _ = r.render_vertices(verts, flame.faces_tensor)
    assert torch.equal(frames, want)
    assert (frames != 255).any()
