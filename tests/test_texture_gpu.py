"""The textured shading pass (csrc/render.hip) against the numpy truth of tests/texture_ref.py.

The reference is fed the GPU's own fp32 screen coordinates, normals and face ids, so no pixel is undecided and none is left out.
The pyramid is compared bit for bit; (u, v, lambda) and the colour under max(16 u, 4 x yardstick), u = 2^-24, the yardstick being
the same restatement run in float32 numpy on the same inputs (render_ref.bound)."""
import functools

import numpy as np
import pytest
import torch

import render_ref as rr
import texture_ref as tr
from msmd_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NEAR = 0.01
T_CENTER = np.array([0.01, -0.02, 0.005], np.float32)
IMAGES = [(64, 64, 1), (37, 53, 3), (130, 70, 1)]           # (W, H, B): B > 1 turns every frame by its own axis-angle
TEXTURES = ["1x1", "5x3", "8x8", "256x256", "256x256-smooth", "64x32-rgba"]
CASES = [(m, W, H, B, t) for m in ("a", "b") for W, H, B in IMAGES for t in TEXTURES]
case_id = lambda c: f"{c[0]}-{c[1]}x{c[2]}-B{c[3]}-{c[4]}"


@functools.lru_cache(maxsize=None)
def mesh(name):
    """(vertices, faces, vt, ft) from test_render_gpu's recipe."""
    if name == "a":            # closed sphere, longitude / latitude coordinates with a seam column and per-triangle poles
        v, f = synth.latlong_sphere(7, 16, 0.09)
        vt, ft = tr.sphere_uv(7, 16)
        assert vt.shape[0] > v.shape[0]
        return v, f, vt, ft
    if name == "b":            # large overlapping triangles, random coordinates per corner in [-1.25, 2.5]
        a = synth.flame_asset()
        f = a["f"][:600].astype(np.int32)
        return (a["v_template"].astype(np.float32), f) + tr.corner_uv("texture/vt_b", f.shape[0])
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def texture(name):
    if name == "256x256-smooth":
        return tr.smooth_texture(256, 256)
    size, _, tag = name.partition("-")
    Ht, Wt = (int(x) for x in size.split("x"))
    return tr.noise_texture(f"texture/{name}", Ht, Wt, 4 if tag == "rgba" else 3)


def rots(B):
    return (0.5 * synth.normalish("render/rot", (3, 3)))[:B].astype(np.float32) if B > 1 else None


def renderer(W, H, **kw):
    from msmd_amd.utils.renderer import MeshRenderer
    return MeshRenderer((W, H), **kw)


def frames(v, B):
    return np.stack([v * np.float32(1.0 + 0.02 * b) for b in range(B)])


@functools.lru_cache(maxsize=None)
def plain(name, W, H, B):
    """The untextured render of a case: (colour, depth, face id) numpy arrays."""
    v, f, _, _ = mesh(name)
    rot = rots(B)
    out = renderer(W, H).render_vertices(torch.from_numpy(frames(v, B)).to(DEV), f, t_center=None if rot is None else T_CENTER,
                                         rot=rot, return_face_id=True)
    return tuple(t.cpu().numpy() for t in out)


@functools.lru_cache(maxsize=None)
def run(name, W, H, B, tex):
    """One textured GPU render of a case and its references, computed once and shared (nothing below modifies them)."""
    v, f, vt, ft = mesh(name)
    img = texture(tex)
    r = renderer(W, H)
    rot = rots(B)
    color, depth, fid, screen, normals, uvl = r.render_vertices(
        torch.from_numpy(frames(v, B)).to(DEV), f, t_center=None if rot is None else T_CENTER, rot=rot, return_face_id=True,
        return_screen=True, tex_img=img, tex_uv={"vt": vt, "ft": ft}, return_uv=True)
    torch.cuda.synchronize()
    _, shade, lights = (t.cpu().numpy() for t in r._device_consts(torch.device(DEV)))
    g = dict(color=color.cpu().numpy(), depth=depth.cpu().numpy(), face_id=fid.cpu().numpy(), screen=screen.cpu().numpy(),
             normals=normals.cpu().numpy(), uvl=uvl.cpu().numpy())
    levels = tr.pyramid(img)
    ref = {dt: [tr.texture_stage(g["screen"][b], g["normals"][b], f, g["face_id"][b], vt, ft, levels, shade, lights, NEAR,
                                 r.bg_color, dt) for b in range(B)] for dt in (np.float64, np.float32)}
    return g, ref


def stacked(rs, key):
    return np.stack([x[key] for x in rs])


def check_against_reference(g, ref, tag):
    """Assertions 3 and 4 of a render `g` against its references; every covered pixel takes part."""
    r64, r32 = ref[np.float64], ref[np.float32]
    covered = g["face_id"] >= 0
    assert covered.any() and np.array_equal(stacked(r64, "covered"), covered)
    assert np.isfinite(g["uvl"]).all() and (g["uvl"][~covered] == 0).all()
    for k, key in enumerate(("u", "v", "lam")):
        g64, g32 = stacked(r64, key)[covered], stacked(r32, key)[covered]
        err = float(rr.rel_err(g["uvl"][..., k][covered], g64).max())
        bnd = rr.bound(g32, g64)
        print(f"{tag} {key}: max err {err / rr.U:.2f} u, bound {bnd / rr.U:.2f} u")
        assert err <= bnd, (key, err / rr.U, bnd / rr.U)
    u8 = stacked(r64, "color_u8")
    off = int(np.abs(g["color"][covered].astype(np.int32) - u8[covered].astype(np.int32)).max())
    # before quantisation, in units of one level (1 / 255): the kernel's unquantised colour is not stored, so its uint8 is held
    # to the reference's unquantised level within the half level rounding costs plus the bound
    lv64, lv32 = 255.0 * stacked(r64, "color")[covered], 255.0 * stacked(r32, "color")[covered].astype(np.float64)
    bnd = rr.bound(lv32, lv64)
    excess = np.abs(g["color"][covered].astype(np.float64) - lv64) - 0.5
    worst = float((excess / np.maximum(1.0, lv64)).max())
    print(f"{tag} colour: {int(covered.sum())} pixels, worst uint8 difference {off}, worst excess over the half level "
          f"{worst / rr.U:.2f} u, bound {bnd / rr.U:.2f} u")
    assert off <= 1
    assert worst <= bnd


# ---------------------------------------------------------------------------------------------- 1. pyramid
@pytest.mark.parametrize("name", TEXTURES + ["1x7", "37x100", "130x3-rgba"])
def test_pyramid_bit_for_bit(name):
    from msmd_amd import ops
    img = texture(name)
    want = tr.flat(tr.pyramid(img))
    got = ops.texture_pyramid(torch.from_numpy(img).to(DEV))
    assert got.dtype == torch.float32 and tuple(got.shape) == want.shape
    assert torch.equal(got.cpu(), torch.from_numpy(want))
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))


# ---------------------------------------------------------------------------------------------- 2. untouched outputs
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_depth_face_id_and_background_are_untouched(case):
    g, _ = run(*case)
    color, depth, fid = plain(*case[:4])
    assert torch.equal(torch.from_numpy(g["depth"]), torch.from_numpy(depth))
    assert torch.equal(torch.from_numpy(g["face_id"]), torch.from_numpy(fid))
    bg = fid < 0
    assert bg.any() and (g["color"][bg] == 255).all() and np.array_equal(g["color"][bg], color[bg])


# ---------------------------------------------------------------------------------------------- 3, 4. (u, v, lambda), colour
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_uv_lod_and_colour(case):
    g, ref = run(*case)
    check_against_reference(g, ref, case_id(case))


def test_the_sphere_cases_reach_both_ends_of_the_pyramid():
    for tex, cond in (("256x256", lambda lam: lam > 1), ("8x8", lambda lam: lam == 0)):
        g, ref = run("a", 64, 64, 1, tex)
        covered = g["face_id"] >= 0
        for lam in (g["uvl"][..., 2][covered], stacked(ref[np.float64], "lam")[covered]):
            assert cond(lam).mean() >= 0.5
    # the random coordinates reach the top level of the small pyramids and stay below it on the large one
    g, _ = run("b", 64, 64, 1, "8x8")
    assert (g["uvl"][..., 2][g["face_id"] >= 0] == 3.0).any()
    g, _ = run("b", 64, 64, 1, "256x256")
    lam = g["uvl"][..., 2][g["face_id"] >= 0]
    assert ((lam > 0) & (lam < 8)).any()
    u = g["uvl"][..., 0][g["face_id"] >= 0]
    assert (u < 0).any() and (u > 1).any()


# ---------------------------------------------------------------------------------------------- 5. constant texture
@pytest.mark.parametrize("name,W,H,B", [("a", 64, 64, 1), ("b", 130, 70, 1)])
def test_constant_texture_is_the_untextured_render_with_that_base_colour(name, W, H, B):
    v, f, vt, ft = mesh(name)
    img = np.full((16, 16, 3), 128, np.uint8)
    verts = torch.from_numpy(frames(v, B)).to(DEV)
    tex, _, fid = renderer(W, H).render_vertices(verts, f, tex_img=img, tex_uv={"vt": vt, "ft": ft}, return_face_id=True)
    r = renderer(W, H)
    r.base_color = np.full(3, 128.0 / 255.0)
    r._consts.clear()
    flat, _ = r.render_vertices(verts, f)
    assert (fid >= 0).any()
    assert int((tex.int() - flat.int()).abs().max()) <= 1
    default, _ = renderer(W, H).render_vertices(verts, f)
    assert not torch.equal(tex, default)


# ---------------------------------------------------------------------------------------------- 6. determinism
def test_determinism_graph_and_batch():
    v, f, vt, ft = mesh("b")
    W, H, B = 130, 70, 3
    r = renderer(W, H)
    verts = torch.from_numpy(frames(v, B)).to(DEV)
    faces = torch.from_numpy(f).to(DEV)
    rot = torch.from_numpy(rots(B)).to(DEV)
    tc = torch.from_numpy(T_CENTER).to(DEV)
    img, uv = texture("256x256"), {"vt": vt, "ft": ft}
    call = lambda vv, rr_: r.render_vertices(vv, faces, t_center=tc, rot=rr_, return_face_id=True, tex_img=img, tex_uv=uv,
                                             return_uv=True)
    first = [t.clone() for t in call(verts, rot)]
    again = call(verts, rot)
    assert len(first) == 4 and all(torch.equal(a, b) for a, b in zip(first, again))
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


# ---------------------------------------------------------------------------------------------- 7. surface
def test_surface():
    from msmd_amd import ops
    v, f, vt, ft = mesh("a")
    img, uv = texture("64x32-rgba"), {"vt": vt.astype(np.float64), "ft": ft.astype(np.int64)}
    r = renderer(37, 53)
    mesh_obj = type("Mesh", (), {"v": v.astype(np.float64), "f": f.astype(np.uint32)})()
    rot = np.array([0.1, 0.3, -0.2])
    color, depth = r.render_mesh(mesh_obj, T_CENTER, rot, tex_img=img, tex_uv=uv)
    assert isinstance(color, np.ndarray) and color.dtype == np.uint8 and color.shape == (53, 37, 3)
    assert isinstance(depth, np.ndarray) and depth.dtype == np.float32 and depth.shape == (53, 37)
    dv = torch.from_numpy(v[None]).to(DEV)
    c2, d2 = r.render_vertices(dv, f, t_center=T_CENTER, rot=rot, tex_img=img, tex_uv=uv)
    assert c2.is_cuda and c2.dtype == torch.uint8 and tuple(c2.shape) == (1, 53, 37, 3)
    assert np.array_equal(c2[0].cpu().numpy(), color) and np.array_equal(d2[0].cpu().numpy(), depth)
    plain_c, _ = r.render_vertices(dv, f, t_center=T_CENTER, rot=rot)
    assert not torch.equal(plain_c, c2)
    # the pyramid and the tables are cached per texture: by contents for arrays, bounded
    n = len(r._tex)
    assert n == 1
    r.render_vertices(dv, f, tex_img=img.copy(), tex_uv={"vt": uv["vt"].copy(), "ft": uv["ft"].copy()})
    assert len(r._tex) == n
    for k in range(6):
        r.render_vertices(dv, f, tex_img=np.full((2, 2, 3), k, np.uint8), tex_uv=uv)
    assert len(r._tex) <= 4
    # a texture without a table, a table without a texture, a table that does not fit
    with pytest.raises(NotImplementedError):
        r.render_vertices(dv, f, tex_img=img)
    with pytest.raises(TypeError):
        r.render_vertices(dv, f, tex_uv=uv)
    with pytest.raises(TypeError):
        r.render_vertices(dv, f, return_uv=True)
    with pytest.raises(ValueError):
        r.render_vertices(dv, f, tex_img=img, tex_uv={"vt": vt, "ft": ft + 1})
    with pytest.raises(ValueError):
        r.render_vertices(dv, f, tex_img=img, tex_uv={"vt": vt, "ft": ft[:-1]})
    with pytest.raises(TypeError):
        r.render_vertices(dv, f, tex_img=img.astype(np.float32), tex_uv=uv)
    # ops take contiguous fp32 / int32 / uint8 CUDA tensors only
    img_d = torch.from_numpy(img).to(DEV)
    for bad in (img_d.cpu(), img_d[:, ::2], img_d.float(), img_d[..., :2].contiguous(), img_d[0]):
        with pytest.raises(TypeError):
            ops.texture_pyramid(bad)
    with pytest.raises(ValueError):
        ops.texture_pyramid(torch.zeros(4097, 1, 3, dtype=torch.uint8, device=DEV))
    pyr = ops.texture_pyramid(img_d)
    faces_d, off, ids = r._tables(f, v.shape[0], dv.device)
    view, shade, lights = r._device_consts(dv.device)
    screen, normals = ops.render_vertices(dv, faces_d, off, ids, view, 1.0 / np.tan(r.fov / 2.0), 53, 37)
    rgba, _, fid = ops.render_raster(screen, normals, faces_d, shade, lights, 53, 37, NEAR, 3.0, 0xffffffff, want_face_id=True)
    vt_d, ft_d = torch.from_numpy(vt).to(DEV), torch.from_numpy(ft).to(DEV)
    good = (screen, normals, faces_d, vt_d, ft_d, pyr, 64, 32, shade, lights, fid, rgba, NEAR)
    before = rgba.clone()
    assert ops.render_shade_textured(*good) is None and not torch.equal(before, rgba)
    uvl = ops.render_shade_textured(*good, want_uvl=True)
    assert uvl.dtype == torch.float32 and tuple(uvl.shape) == (1, 53, 37, 3)
    for k, bad in ((0, screen.cpu()), (1, normals[:, ::2]), (2, faces_d.long()), (3, vt_d.double()), (3, vt_d.t()), (4, ft_d.long()),
                   (4, ft_d[:-1]), (5, pyr.cpu()), (5, pyr[:-1]), (5, pyr.double()), (8, shade[:3]), (9, lights.t()),
                   (10, fid.long()), (10, fid.cpu()), (11, rgba[..., :3]), (11, rgba.int())):
        args = list(good)
        args[k] = bad
        with pytest.raises(TypeError):
            ops.render_shade_textured(*args)
    # the kernel never reads outside vt: an index outside [0, Nt) (which the host refuses) counts as the coordinate (0, 0)
    bad_ft = ft.copy()
    bad_ft[::3, 1] = vt.shape[0] + 5
    bad_ft[1::3, 2] = -1
    fixed_ft = np.where((bad_ft < 0) | (bad_ft >= vt.shape[0]), vt.shape[0], bad_ft).astype(np.int32)
    vt0 = torch.from_numpy(np.concatenate([vt, np.zeros((1, 2), np.float32)])).to(DEV)
    got, want = rgba.clone(), rgba.clone()
    a = ops.render_shade_textured(screen, normals, faces_d, vt_d, torch.from_numpy(bad_ft).to(DEV), pyr, 64, 32, shade, lights, fid,
                                  got, NEAR, want_uvl=True)
    b = ops.render_shade_textured(screen, normals, faces_d, vt0, torch.from_numpy(fixed_ft).to(DEV), pyr, 64, 32, shade, lights, fid,
                                  want, NEAR, want_uvl=True)
    assert torch.equal(a, b) and torch.equal(got, want) and not torch.equal(a, uvl)


# ---------------------------------------------------------------------------------------------- 8. non-finite coordinates
def test_non_finite_coordinates_count_as_zero():
    v, f, vt, ft = mesh("a")
    vt = vt.copy()
    vt[3::11, 0] = np.nan
    vt[5::13, 1] = np.inf
    vt[7::17] = (-np.inf, np.nan)
    img = texture("256x256")
    W, H = 64, 64
    r = renderer(W, H)
    color, depth, fid, screen, normals, uvl = r.render_vertices(torch.from_numpy(v[None]).to(DEV), f, return_face_id=True,
                                                                return_screen=True, tex_img=img, tex_uv={"vt": vt, "ft": ft},
                                                                return_uv=True)
    torch.cuda.synchronize()
    _, shade, lights = (t.cpu().numpy() for t in r._device_consts(torch.device(DEV)))
    g = dict(color=color.cpu().numpy(), face_id=fid.cpu().numpy(), uvl=uvl.cpu().numpy())
    levels = tr.pyramid(img)
    ref = {dt: [tr.texture_stage(screen[0].cpu().numpy(), normals[0].cpu().numpy(), f, g["face_id"][0], vt, ft, levels, shade,
                                 lights, NEAR, r.bg_color, dt)] for dt in (np.float64, np.float32)}
    covered = g["face_id"] >= 0
    clean = run("a", W, H, 1, "256x256")[0]["uvl"]
    hit = covered & ((g["uvl"][..., 0] != clean[..., 0]) | (g["uvl"][..., 1] != clean[..., 1]))
    print(f"{int(hit.sum())} of {int(covered.sum())} covered pixels lie in a face with a coordinate that is not finite")
    assert hit.sum() >= 0.1 * covered.sum() and (~hit & covered).sum() >= 0.1 * covered.sum()
    assert (g["uvl"][..., 2][hit] == 0).all()             # no derivative there: level 0
    check_against_reference(g, ref, "non-finite vt")


# ---------------------------------------------------------------------------------------------- 9. render_coeffs
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
    vt, ft = tr.corner_uv("texture/vt_flame", flame.faces_tensor.shape[0], 0.0, 1.0)
    img, uv = texture("256x256-smooth"), {"vt": vt, "ft": ft}
    r = renderer(64, 64)
    frames_ = render_coeffs(coef, shape, flame, None, r, chunk=2, tex_img=img, tex_uv=uv)          # two chunks
    assert frames_.dtype == torch.uint8 and tuple(frames_.shape) == (T, 64, 64, 3) and frames_.is_cuda
    verts = coef_dict_to_vertices(get_coef_dict(coef, shape.expand(T, -1), None, with_global_pose=True), flame)
    want, _ = r.render_vertices(verts, flame.faces_tensor, tex_img=img, tex_uv=uv)
    assert torch.equal(frames_, want)
    plain_frames, _ = r.render_vertices(verts, flame.faces_tensor)
    assert not torch.equal(frames_, plain_frames)
    assert len(r._tex) == 1
