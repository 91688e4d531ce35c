"""The four-sample renderer (csrc/render.hip, MeshRenderer(samples=4)) against the numpy truth of
tests/render_msaa_ref.py.

As in test_render_gpu, the reference's raster stage is fed the GPU's own fp32 screen coordinates and normals, so coverage is compared
exactly, sample by sample; depth is held to render_ref.bound = max(16 u, 4 x the float32 yardstick); a resolved byte to 1 level, since
each sample's byte is within 1 level, their sum within 4 and (sum + 2) >> 2 within 1."""
import functools

import numpy as np
import pytest
import torch

import render_msaa_ref as mr
import render_ref as rr
import texture_ref as tr
from msmd_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NEAR, FAR = 0.01, 3.0
T_CENTER = np.array([0.01, -0.02, 0.005], np.float32)
WHITE, CLEAR = 0xffffffff, 0x00000000

# (mesh, W, H, B): 130 x 70 straddles a 32- and a 64-pixel tile grid, 33 x 31 puts an image edge one pixel past a tile edge, `b`
# has the faces whose box goes to the wave walk, every face of `d` meets the one tile so the compacted list is flushed mid-stream
CASES = [("a", 37, 53, 3), ("a", 130, 70, 1), ("b", 130, 70, 3), ("b", 64, 64, 1), ("c", 37, 53, 1), ("d", 31, 29, 1), ("a", 33, 31, 1)]
case_id = lambda c: f"{c[0]}-{c[1]}x{c[2]}-B{c[3]}"


@functools.lru_cache(maxsize=None)
def mesh(name):
    if name == "a":            # small closed sphere
        return synth.latlong_sphere(7, 16, 0.09)
    if name == "b":            # large overlapping triangles, heavy overdraw
        a = synth.flame_asset()
        return a["v_template"].astype(np.float32), a["f"][:600].astype(np.int32)
    if name == "c":            # sub-pixel triangles: many cover no sample
        return synth.latlong_sphere(49, 100, 0.09)
    if name == "d":            # 5184 faces in one tile: more than the compacted list holds
        return synth.latlong_sphere(36, 72, 0.09)
    raise KeyError(name)


def rots(B):
    return (0.5 * synth.normalish("render/rot", (3, 3)))[:B].astype(np.float32) if B > 1 else None


def frames(v, B):
    return np.stack([v * np.float32(1.0 + 0.02 * b) for b in range(B)])


def renderer(W, H, **kw):
    from msmd_amd.utils.renderer import MeshRenderer
    return MeshRenderer((W, H), **kw)


def raster(r, screen, normals, faces_d, background, **kw):
    from msmd_amd import ops
    _, shade, lights = r._device_consts(screen.device)
    return ops.render_raster(screen, normals, faces_d, shade, lights, r.height, r.width, NEAR, FAR, background, **kw)


@functools.lru_cache(maxsize=None)
def run(name, W, H, B):
    """One four-sample GPU render of a case and its references, computed once and shared (nothing below modifies them)."""
    v, f = mesh(name)
    r = renderer(W, H, samples=4)
    verts, rot = torch.from_numpy(frames(v, B)).to(DEV), rots(B)
    color, depth, fid, screen, normals = r.render_vertices(verts, f, t_center=None if rot is None else T_CENTER, rot=rot,
                                                           return_face_id=True, return_screen=True)
    faces_d = r._tables(f, v.shape[0], verts.device)[0]
    rgba, depth2, fid2, sdepth = raster(r, screen, normals, faces_d, WHITE, want_face_id=True, samples=4, want_sample_depth=True)
    clear = raster(r, screen, normals, faces_d, CLEAR, samples=4)[0]
    one = renderer(W, H).render_vertices(verts, f, t_center=None if rot is None else T_CENTER, rot=rot)[0]
    torch.cuda.synchronize()
    assert torch.equal(rgba[..., :3], color) and torch.equal(depth, depth2) and torch.equal(fid, fid2)
    _, shade, lights = (t.cpu().numpy() for t in r._device_consts(torch.device(DEV)))
    g = dict(rgba=rgba.cpu().numpy(), depth=depth.cpu().numpy(), face_id=fid.cpu().numpy(), sample_depth=sdepth.cpu().numpy(),
             clear=clear.cpu().numpy(), one=one.cpu().numpy(), screen=screen.cpu().numpy(), normals=normals.cpu().numpy())
    rs = {dt: [mr.raster_samples(g["screen"][b], g["normals"][b], f, H, W, NEAR, FAR, shade, lights, r.bg_color, mr.SAMPLES4, dt)
               for b in range(B)] for dt in (np.float64, np.float32)}
    return g, rs


def stacked(rs, key):
    return np.stack([x[key] for x in rs])


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_coverage_face_id_depth_and_resolve(case):
    g, rs = run(*case)
    r64, r32 = rs[np.float64], rs[np.float32]
    fid64 = stacked(r64, "face_id")
    covered = fid64 >= 0
    assert g["face_id"].shape == covered.shape == case[3:] + (case[2], case[1], 4) and covered.any()
    # the covered-sample set is exact
    assert np.array_equal(g["face_id"] >= 0, covered)
    # the winning face per sample, outside the samples the reference cannot decide
    amb = np.stack([mr.ambiguous(x) for x in r64])
    print(f"{case}: {int(covered.sum())} covered samples, {int(amb.sum())} undecided")
    assert amb.sum() <= 0.005 * covered.sum()
    sure = covered & ~amb
    assert np.array_equal(g["face_id"][sure], fid64[sure])
    # per-sample depth where the winner is decided (and the float32 restatement agrees on it); 0 on an uncovered sample
    sure32 = sure & (stacked(r32, "face_id") == fid64)
    d64, d32 = stacked(r64, "depth"), stacked(r32, "depth")
    err = float(rr.rel_err(g["sample_depth"][sure32], d64[sure32]).max())
    bnd = rr.bound(d32[sure32], d64[sure32])
    print(f"{case} sample depth: max err {err / rr.U:.2f} u, bound {bnd / rr.U:.2f} u")
    assert err <= bnd
    assert (g["sample_depth"][~covered] == 0.0).all() and (g["face_id"][~covered] == -1).all()
    # the pixel's depth: the least of the kernel's own sample depths over the covered samples, bit for bit; 0 where there are none
    least = np.where(covered, g["sample_depth"], np.float32(np.inf)).min(-1)
    least = np.where(covered.any(-1), least, np.float32(0)).astype(np.float32)
    assert np.array_equal(g["depth"].view(np.uint32), least.view(np.uint32))
    # the resolved colour on pixels whose four samples are all decided: within 1 level of the reference's resolved bytes
    want = mr.resolve(stacked(r64, "color_u8"), covered, (255, 255, 255, 255))
    decided = ~amb.any(-1)
    off = np.abs(g["rgba"].astype(np.int32) - want.astype(np.int32))
    print(f"{case} resolve: {int(decided.sum())} decided pixels, worst difference {int(off[decided].max())} level, "
          f"{int((off[decided] > 0).any(-1).sum())} pixels differ")
    assert off[decided].max() <= 1
    # no covered sample: the background exactly; alpha is 255 everywhere under an opaque background
    none = ~covered.any(-1)
    assert none.any() and (g["rgba"][none] == 255).all() and (g["rgba"][..., 3] == 255).all()
    # four samples on one face: within 1 level of the mean of that face's four unquantised sample levels (each byte is within
    # 0.5 + e of its level, so their mean is, and the rounded mean adds at most 0.5; e, the float32 error of a level, is far
    # below the 1e-3 allowed here)
    same = decided & covered.all(-1) & (g["face_id"] == g["face_id"][..., :1]).all(-1)
    mean = 255.0 * stacked(r64, "color").mean(-2)
    worst = float(np.abs(g["rgba"][..., :3][same].astype(np.float64) - mean[same]).max()) if same.any() else 0.0
    print(f"{case} one-face pixels: {int(same.sum())}, worst distance from the four-sample mean {worst:.4f} level")
    assert same.any() or case[0] in "cd"              # the faces of `c` and `d` are smaller than a pixel
    assert worst <= 1.0 + 1e-3
    # a background alpha of 0: the stored alpha is the coverage, and the colour bytes are the covered samples' sum
    assert np.array_equal(g["clear"][..., 3], ((255 * covered.sum(-1) + 2) >> 2).astype(np.uint8))
    full = covered.all(-1)
    assert np.array_equal(g["clear"][full], g["rgba"][full]) and (g["clear"][none] == 0).all()


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_partly_covered_pixels_are_blended(case):
    """The assertion that anti-aliasing happened: every case has pixels with one to three covered samples, and there the four-sample
    image is not the one-sample image.  A pixel can coincide, for instance where a face is clamped to the white of the background
    under the five lights: such pixels are counted, printed and capped at a tenth of the partly covered ones (on an MI355X: none
    on the spheres, 24 of 1 078 and 1 of 214 on the two `b` cases)."""
    g, rs = run(*case)
    n = (g["face_id"] >= 0).sum(-1)
    part = (n > 0) & (n < 4)
    differ = (g["rgba"][..., :3] != g["one"]).any(-1)
    print(f"{case}: {int(part.sum())} partly covered pixels, the two images differ on {int((part & differ).sum())} of them and on "
          f"{int((~part & differ).sum())} others")
    assert part.sum() > 0
    assert (part & differ).sum() >= 0.9 * part.sum()
    # (a pixel with no covered sample can still differ: a sliver through its centre covers none of the four samples)


def test_one_sample_through_the_new_arguments_is_the_existing_call():
    from msmd_amd import _lib
    v, f = mesh("b")
    W, H, B = 130, 70, 3
    r = renderer(W, H)
    verts, rot = torch.from_numpy(frames(v, B)).to(DEV), rots(B)
    color, depth, fid, screen, normals = r.render_vertices(verts, f, t_center=T_CENTER, rot=rot, return_face_id=True, return_screen=True)
    faces_d = r._tables(f, v.shape[0], verts.device)[0]
    old = raster(r, screen, normals, faces_d, WHITE, want_face_id=True)
    new = raster(r, screen, normals, faces_d, WHITE, want_face_id=True, samples=1, want_sample_depth=True)
    assert len(old) == 3 and len(new) == 4
    assert torch.equal(old[0][..., :3], color) and torch.equal(old[1], depth) and torch.equal(old[2], fid)
    assert torch.equal(new[0], old[0]) and torch.equal(new[1], old[1])
    assert torch.equal(new[2].reshape(B, H, W), old[2]) and torch.equal(new[3].reshape(B, H, W), old[1])
    assert renderer(W, H, samples=1).samples == 1
    same = renderer(W, H, samples=1).render_vertices(verts, f, t_center=T_CENTER, rot=rot, return_face_id=True)
    assert all(torch.equal(a, b) for a, b in zip(same, (color, depth, fid)))
    # any other sample count is refused before anything is launched: the buffers keep what they held
    lib = _lib.load()
    _, shade, lights = r._device_consts(verts.device)
    rgba = torch.full((B, H, W, 4), 7, dtype=torch.uint8, device=DEV)
    d = torch.full((B, H, W), 7.0, device=DEV)
    for samples in (0, 2, 3, 8, -4):
        rc = lib.msmd_render_raster_ms(screen.data_ptr(), normals.data_ptr(), faces_d.data_ptr(), shade.data_ptr(), lights.data_ptr(),
                                       lights.shape[0], rgba.data_ptr(), d.data_ptr(), None, None, B, v.shape[0], faces_d.shape[0],
                                       H, W, NEAR, FAR, WHITE, samples, torch.cuda.current_stream().cuda_stream)
        assert rc == 1
    torch.cuda.synchronize()
    assert (rgba == 7).all() and (d == 7.0).all()
    from msmd_amd import ops
    with pytest.raises(ValueError):
        ops.render_raster(screen, normals, faces_d, shade, lights, H, W, NEAR, FAR, WHITE, samples=2)


def test_determinism_and_batch():
    v, f = mesh("b")
    W, H, B = 130, 70, 3
    r = renderer(W, H, samples=4)
    verts = torch.from_numpy(frames(v, B)).to(DEV)
    faces = torch.from_numpy(f).to(DEV)
    rot = torch.from_numpy(rots(B)).to(DEV)
    tc = torch.from_numpy(T_CENTER).to(DEV)
    call = lambda vv, rr_: r.render_vertices(vv, faces, t_center=tc, rot=rr_, return_face_id=True)
    first = [t.clone() for t in call(verts, rot)]
    again = call(verts, rot)
    assert tuple(first[2].shape) == (B, H, W, 4)
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    for b in range(B):                                  # a frame of the batch equals that frame rendered alone
        alone = call(verts[b:b + 1].contiguous(), rot[b:b + 1].contiguous())
        assert all(torch.equal(a[b:b + 1], x) for a, x in zip(first, alone))


def test_degenerate_inputs_draw_nothing():
    r = renderer(64, 64, samples=4)
    nan = float("nan")
    v = np.array([[-0.05, -0.05, 0], [0.05, -0.05, 0], [0, 0.05, 0],      # 0-2: a visible triangle
                  [0, 0, 0.995], [0.001, 0, 0.995], [0, 0.001, 0.995],    # 3-5: nearer than `near` (depth 0.005)
                  [5, 5, 0], [5.1, 5, 0], [5, 5.1, 0],                    # 6-8: far off-screen
                  [nan, 0, 0]], np.float32)                               # 9: not a number
    V = v.shape[0]
    dv = torch.from_numpy(v[None]).to(DEV)
    # the vertex stage over faces that leave the visible triangle's normals alone; the raster stage over the lists under test
    screen, normals = r.render_vertices(dv, np.array([[0, 1, 2], [3, 4, 5], [6, 7, 8], [9, 9, 9]], np.int32), return_screen=True)[2:]
    full = np.array([[0, 1, 2], [0, 0, 1], [3, 4, 5], [6, 7, 8], [0, 1, 9], [0, 1, V], [0, -1, 2]], np.int32)
    go = lambda faces: raster(r, screen, normals, torch.from_numpy(np.ascontiguousarray(faces)).to(DEV), WHITE, want_face_id=True,
                              samples=4, want_sample_depth=True)
    want = go(full[:1])                                # F = 1
    ids = want[2].cpu().numpy()
    assert set(np.unique(ids)) == {-1, 0}
    n = (ids >= 0).sum(-1)
    assert (n == 4).any() and ((n > 0) & (n < 4)).any() and (n == 0).any()
    got = go(full)                                     # with the faces that must draw nothing
    assert all(torch.equal(a, b) for a, b in zip(want, got))
    rgba, depth, ids, sdepth = go(full[1:])            # nothing visible
    assert (ids == -1).all() and (depth == 0).all() and (sdepth == 0).all() and (rgba == 255).all()
    cb = renderer(64, 64, black_bg=True, samples=4).render_vertices(dv, full[3:4])[0]
    assert (cb == 0).all()


# ---------------------------------------------------------------------------------------------- textured
@functools.lru_cache(maxsize=None)
def run_textured(name, W, H):
    v, f = mesh(name)
    if name == "a":
        vt, ft = tr.sphere_uv(7, 16)
    else:
        vt, ft = tr.corner_uv("texture/vt_b", f.shape[0])
    img = tr.noise_texture("msaa/texture", 8, 16)
    r = renderer(W, H, samples=4)
    dv = torch.from_numpy(v[None]).to(DEV)
    plain = r.render_vertices(dv, f)[0]
    color, depth, fid, screen, normals = r.render_vertices(dv, f, return_face_id=True, return_screen=True, tex_img=img,
                                                           tex_uv={"vt": vt, "ft": ft})
    torch.cuda.synchronize()
    _, shade, lights = (t.cpu().numpy() for t in r._device_consts(torch.device(DEV)))
    g = dict(color=color.cpu().numpy()[0], plain=plain.cpu().numpy()[0], face_id=fid.cpu().numpy()[0], screen=screen.cpu().numpy()[0],
             normals=normals.cpu().numpy()[0])
    ref = mr.raster_samples(g["screen"], g["normals"], f, H, W, NEAR, FAR, shade, lights, r.bg_color)
    tex = mr.texture_samples(g["screen"], g["normals"], f, g["face_id"], vt, ft, tr.pyramid(img), shade, lights, NEAR)
    return g, ref, tex


@pytest.mark.parametrize("name,W,H", [("a", 37, 53), ("b", 64, 64)])
def test_textured_resolve(name, W, H):
    """The textured restatement is fed the GPU's sample face ids (as test_texture_gpu feeds it the GPU's face ids) and compared on the
    pixels whose four samples the raster reference decides, where those ids are the reference's.  test_texture_gpu leaves no pixel
    out for a level of detail near an integer (the trilinear blend is continuous there), and neither does this."""
    g, ref, tex = run_textured(name, W, H)
    covered = ref["face_id"] >= 0
    assert np.array_equal(g["face_id"] >= 0, covered) and np.array_equal(tex["covered"], covered)
    decided = ~mr.ambiguous(ref).any(-1)
    assert np.array_equal(g["face_id"][decided], ref["face_id"][decided])
    want = mr.resolve(tex["color_u8"], covered, (255, 255, 255, 255))[..., :3]
    some = covered.any(-1)
    off = np.abs(g["color"].astype(np.int32) - want.astype(np.int32))
    print(f"{name} {W}x{H} textured: {int((decided & some).sum())} decided pixels with a covered sample, worst difference "
          f"{int(off[decided & some].max())} level; level of detail up to {float(tex['lam'].max()):.2f}")
    assert (decided & some).any() and off[decided & some].max() <= 1
    # no covered sample: left as the raster pass wrote it
    assert (~some).any() and np.array_equal(g["color"][~some], g["plain"][~some]) and (g["color"][~some] == 255).all()
    assert (g["color"][some] != g["plain"][some]).any()
    part = some & ~covered.all(-1)
    assert part.any()


# ---------------------------------------------------------------------------------------------- surface
def test_surface():
    from msmd_amd import ops
    v, f = mesh("a")
    r = renderer(37, 53, samples=4)
    mesh_obj = type("Mesh", (), {"v": v.astype(np.float64), "f": f.astype(np.uint32)})()
    rot = np.array([0.1, 0.3, -0.2])
    color, depth = r.render_mesh(mesh_obj, T_CENTER, rot)
    assert isinstance(color, np.ndarray) and color.dtype == np.uint8 and color.shape == (53, 37, 3)
    assert isinstance(depth, np.ndarray) and depth.dtype == np.float32 and depth.shape == (53, 37)
    one, _ = renderer(37, 53).render_mesh(mesh_obj, T_CENTER, rot)
    assert not np.array_equal(one, color) and (depth > 0).any() and (depth == 0).any()
    dv = torch.from_numpy(v[None]).to(DEV)
    c2, d2, fid = r.render_vertices(dv, f, t_center=T_CENTER, rot=rot, return_face_id=True)
    assert tuple(c2.shape) == (1, 53, 37, 3) and tuple(fid.shape) == (1, 53, 37, 4) and fid.dtype == torch.int32
    assert np.array_equal(c2[0].cpu().numpy(), color) and np.array_equal(d2[0].cpu().numpy(), depth)
    with pytest.raises(ValueError):
        renderer(37, 53, samples=2)
    vt, ft = tr.sphere_uv(7, 16)
    img, uv = tr.noise_texture("msaa/texture", 8, 16), {"vt": vt, "ft": ft}
    with pytest.raises(ValueError):
        r.render_vertices(dv, f, tex_img=img, tex_uv=uv, return_uv=True)
    tex, _ = r.render_mesh(mesh_obj, T_CENTER, rot, tex_img=img, tex_uv=uv)
    assert tex.shape == (53, 37, 3) and not np.array_equal(tex, color)
    # the textured wrapper at four samples: (B, H, W, 4) ids, the background, no uvl
    faces_d = r._tables(f, v.shape[0], dv.device)[0]
    _, shade, lights = r._device_consts(dv.device)
    screen, normals = r.render_vertices(dv, f, return_screen=True)[2:]
    rgba, _, ids = raster(r, screen, normals, faces_d, WHITE, want_face_id=True, samples=4)
    pyr = ops.texture_pyramid(torch.from_numpy(img).to(DEV))
    vt_d, ft_d = torch.from_numpy(vt).to(DEV), torch.from_numpy(ft).to(DEV)
    good = (screen, normals, faces_d, vt_d, ft_d, pyr, 8, 16, shade, lights, ids, rgba, NEAR)
    before = rgba.clone()
    assert ops.render_shade_textured(*good, samples=4, background=WHITE) is None and not torch.equal(before, rgba)
    with pytest.raises(ValueError):
        ops.render_shade_textured(*good, samples=4)                             # no background
    with pytest.raises(ValueError):
        ops.render_shade_textured(*good, samples=4, background=WHITE, want_uvl=True)
    with pytest.raises(ValueError):
        ops.render_shade_textured(*good, samples=3, background=WHITE)
    with pytest.raises(TypeError):
        ops.render_shade_textured(*good)                                        # four-sample ids at one sample
    with pytest.raises(TypeError):
        ops.render_shade_textured(*good[:10], ids[..., 0].contiguous(), rgba, NEAR, samples=4, background=WHITE)


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
    r = renderer(64, 64, samples=4)
    frames_ = render_coeffs(coef, shape, flame, None, r, chunk=2)          # two chunks
    assert frames_.dtype == torch.uint8 and tuple(frames_.shape) == (T, 64, 64, 3) and frames_.is_cuda
    verts = coef_dict_to_vertices(get_coef_dict(coef, shape.expand(T, -1), None, with_global_pose=True), flame)
    want, _ = r.render_vertices(verts, flame.faces_tensor)
    assert torch.equal(frames_, want)
    one, _ = renderer(64, 64).render_vertices(verts, flame.faces_tensor)
    assert not torch.equal(frames_, one) and (frames_ != 255).any()


def test_four_sample_frames_make_a_playable_video(tmp_path):
    """The --video branch of inference.main with a four-sample renderer, from the coefficients on: render_coeffs_chunks ->
    media.encode_jpeg -> media.write_avi, read back by the project's own AVI reader and JPEG decoder."""
    from types import SimpleNamespace
    from msmd_amd.inference import render_coeffs_chunks
    from msmd_amd.utils import media
    from msmd_amd.utils.flame import FLAME, FLAMEConfig
    cfg = SimpleNamespace(**vars(FLAMEConfig))
    cfg.asset = synth.flame_asset()
    flame = FLAME(cfg).to(DEV)
    T, N = 5, 64
    coef = torch.from_numpy(0.3 * synth.normalish("render/coef", (T, 54))).float().to(DEV)
    shape = torch.from_numpy(0.3 * synth.normalish("render/shape", (1, 100))).float().to(DEV)
    sizes = {}
    for samples in (4, 1):
        r = renderer(N, N, samples=samples)
        parts = list(render_coeffs_chunks(coef, shape, flame, None, r, chunk=2))
        jpegs = [j for part in parts for j in media.encode_jpeg(part, 90)]
        sizes[samples] = sum(len(j) for j in jpegs)
        if samples == 4:
            path = tmp_path / "msaa.avi"
            media.write_avi(path, jpegs, 25, (N, N), None)
            frames4 = torch.cat(parts)
    back = media.read_video(path, device=DEV)
    assert tuple(back.shape) == (T, N, N, 3) and back.dtype == torch.uint8
    mse = float(((back.float() - frames4.float()) ** 2).mean())
    psnr = 10 * np.log10(255.0 ** 2 / mse)
    print(f"{T} frames of {N} x {N} at quality 90: {sizes[4]} bytes of JPEG at four samples, {sizes[1]} at one; PSNR of the file "
          f"against the rendered frames {psnr:.2f} dB")
    assert psnr > 30.0 and len(media.read_avi(path).frames) == T
