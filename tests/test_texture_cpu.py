"""The texture pass's numpy truth (tests/texture_ref.py) pinned by closed forms, and the host-side code that needs no GPU: the
texture validator and the command line.  The last test confirms on the CPU the conditions tests/test_texture_gpu.py puts on
its sphere cases (which levels of the pyramid they reach)."""
import numpy as np
import pytest

import render_ref as rr
import texture_ref as tr

SHADE = np.array([0.3, 0.3, 0.3, 0.2, 0.2, 0.2], np.float32)
LIGHTS = np.array([[0, 0, 1, 2.0]] * 5, np.float32)
BG = (255, 255, 255)


def _img(Ht, Wt, seed=0, channels=3):
    return np.random.default_rng(seed).integers(0, 256, size=(Ht, Wt, channels), dtype=np.uint8)


def test_pyramid_sizes_and_values_1x1_2x2_5x3():
    one = np.array([[[7, 8, 9]]], np.uint8)
    lv = tr.pyramid(one)
    assert tr.level_sizes(1, 1) == [(1, 1)] and len(lv) == 1 and lv[0].dtype == np.float32
    assert np.array_equal(lv[0], [[[7, 8, 9, 0]]])
    two = np.array([[[1, 0, 0], [2, 0, 0]], [[4, 0, 0], [9, 0, 255]]], np.uint8)
    lv = tr.pyramid(two)
    assert tr.level_sizes(2, 2) == [(2, 2), (1, 1)]
    assert np.array_equal(lv[1], [[[4.0, 0, 63.75, 0]]])
    # 5 rows x 3 columns -> 2 x 1 -> 1 x 1: row 4 and column 2 are never read, and the 2 x 1 level's right neighbour is clamped
    img = _img(5, 3, 1)
    lv = tr.pyramid(img)
    assert tr.level_sizes(5, 3) == [(5, 3), (2, 1), (1, 1)] and [l.shape for l in lv] == [(5, 3, 4), (2, 1, 4), (1, 1, 4)]
    f = img.astype(np.float64)
    for y in range(2):
        want = (f[2 * y, 0] + f[2 * y, 1] + f[2 * y + 1, 0] + f[2 * y + 1, 1]) / 4          # exact: sums of four bytes
        assert np.array_equal(lv[1][y, 0, :3], want)
    want = ((lv[1][0, 0] + lv[1][0, 0]) + (lv[1][1, 0] + lv[1][1, 0])) * np.float32(0.25)
    assert np.array_equal(lv[2][0, 0], want)
    changed = img.copy()
    changed[4, :] ^= 0xff
    changed[:, 2] ^= 0xff
    assert all(np.array_equal(a, b) for a, b in zip(lv[1:], tr.pyramid(changed)[1:]))
    # alpha is ignored; the flat layout is the levels one after the other
    rgba = np.concatenate([img, _img(5, 3, 2, 1)], axis=-1)
    assert np.array_equal(tr.flat(tr.pyramid(rgba)), tr.flat(lv)) and tr.flat(lv).shape == (15 + 2 + 1, 4)
    assert len(tr.level_sizes(4096, 1)) == 13 and len(tr.level_sizes(37, 100)) == 7


def test_constant_texture_gives_its_constant_anywhere():
    img = np.empty((6, 10, 3), np.uint8)
    img[...] = (31, 128, 250)
    lv = tr.pyramid(img)
    u = np.array([-3.7, -1.0, -0.2, 0.0, 0.49, 1.0, 1.3, 17.25])
    v = np.array([5.5, -0.01, 0.0, 1.0, 0.99, -2.25, 0.5, 0.123])
    for lam in (0.0, 0.3, 1.0, 2.5, len(lv) - 1.0):
        T = tr.sample(lv, u, v, np.full(u.shape, lam))
        assert np.abs(T - np.array([31.0, 128.0, 250.0])).max() < 1e-12


def test_texel_centres_wrap_and_the_v_axis():
    img = _img(5, 7, 3)
    lv = tr.pyramid(img)
    y, x = np.mgrid[0:5, 0:7]
    u, v = (x.ravel() + 0.5) / 7, 1.0 - (y.ravel() + 0.5) / 5          # row 0 is the top of the image: v = 1
    T = tr.sample_level(lv[0], u, v)
    assert np.abs(T - img.reshape(-1, 3)).max() < 1e-11
    # the same one period to the left and three up
    assert np.abs(tr.sample_level(lv[0], u - 1.0, v + 3.0) - img.reshape(-1, 3)).max() < 1e-10
    # continuity across the wrap: u = 1 - eps and u = 1 + eps agree to O(eps)
    eps = 1e-7
    vv = np.linspace(0.05, 0.95, 7)
    a, b = tr.sample_level(lv[0], np.full(7, 1 - eps), vv), tr.sample_level(lv[0], np.full(7, 1 + eps), vv)
    assert np.abs(a - b).max() <= 2 * eps * 7 * 255
    a, b = tr.sample_level(lv[0], vv, np.full(7, 1 - eps)), tr.sample_level(lv[0], vv, np.full(7, 1 + eps))
    assert np.abs(a - b).max() <= 2 * eps * 5 * 255
    # u = 0 lies half way between the last and the first column, v = 0 half way between the bottom and the top row
    uc = (np.arange(7) + 0.5) / 7
    T = tr.sample_level(lv[0], uc, np.zeros(7))
    assert np.abs(T - 0.5 * (img[4].astype(np.float64) + img[0])).max() < 1e-11
    vc = 1.0 - (np.arange(5) + 0.5) / 5
    T = tr.sample_level(lv[0], np.zeros(5), vc)
    assert np.abs(T - 0.5 * (img[:, 6].astype(np.float64) + img[:, 0])).max() < 1e-11
    # not finite -> 0
    bad = tr.sample_level(lv[0], np.array([np.nan, np.inf, -np.inf]), np.array([0.3, np.nan, 0.3]))
    want = tr.sample_level(lv[0], np.zeros(3), np.array([0.3, 0.0, 0.3]))
    assert np.array_equal(bad, want)
    # trilinear: half way between two levels
    T = tr.sample(lv, uc, np.full(7, 0.4), np.full(7, 0.5))
    assert np.abs(T - 0.5 * (tr.sample_level(lv[0], uc, np.full(7, 0.4)) + tr.sample_level(lv[1], uc, np.full(7, 0.4)))).max() < 1e-11
    # the float32 restatement stays float32
    assert tr.sample(lv, uc, vc[[0, 1, 2, 3, 4, 0, 1]], np.full(7, 0.5), np.float32).dtype == np.float32


def _quad(n, depth=1.0):
    """Two triangles over the pixels [0, n)^2, facing the camera."""
    s = np.array([[0, 0, depth], [n, 0, depth], [0, n, depth], [n, n, depth]], np.float32)
    return s, np.tile(np.array([[0, 0, 1]], np.float32), (4, 1)), np.array([[0, 1, 2], [1, 3, 2]])


@pytest.mark.parametrize("r", [0.25, 1.0, 2.0, 3.0, 8.0, 100.0])
def test_fronto_parallel_quad_at_r_texels_per_pixel(r):
    n, Ht, Wt = 16, 32, 64
    s, nrm, faces = _quad(n)
    fid = rr.raster_stage(s, nrm, faces, n, n, 0.01, 3.0, SHADE, LIGHTS, BG)["face_id"]
    assert (fid >= 0).all()
    lv = tr.pyramid(_img(Ht, Wt, 4))
    L = len(lv)
    assert L == 7
    # u runs along x at r texels of the 64-wide image per pixel; v is constant, then runs along y at r texels of the 32 rows
    for vt in (np.array([[0, 0.5], [n * r / Wt, 0.5], [0, 0.5], [n * r / Wt, 0.5]]),
               np.array([[0.25, 0], [0.25, 0], [0.25, -n * r / Ht], [0.25, -n * r / Ht]])):
        for dt, tol in ((np.float64, 1e-12), (np.float32, 1e-4)):
            out = tr.texture_stage(s, nrm, faces, fid, vt.astype(np.float32), faces, lv, SHADE, LIGHTS, 0.01, BG, dt)
            assert out["lam"].dtype == dt
            want = min(max(np.log2(r), 0.0), L - 1.0)
            assert np.abs(out["lam"] - want).max() <= tol, (r, float(np.abs(out["lam"] - want).max()))
    # the interpolated coordinate itself: u at the centre of pixel j is (j + 0.5) r / Wt
    out = tr.texture_stage(s, nrm, faces, fid, np.array([[0, 0.5], [n * r / Wt, 0.5], [0, 0.5], [n * r / Wt, 0.5]], np.float32),
                           faces, lv, SHADE, LIGHTS, 0.01, BG)
    assert np.abs(out["u"] - (np.arange(n) + 0.5)[None, :] * np.float32(n * r / Wt) / n).max() < 1e-12
    assert np.abs(out["v"] - 0.5).max() < 1e-15


def test_texture_stage_orientation_bad_indices_and_shading():
    n = 8
    s, nrm, faces = _quad(n)
    fid = rr.raster_stage(s, nrm, faces, n, n, 0.01, 3.0, SHADE, LIGHTS, BG)["face_id"]
    img = np.empty((4, 4, 3), np.uint8)
    img[...] = (64, 128, 255)
    lv = tr.pyramid(img)
    vt = np.array([[0, 1], [1, 1], [0, 0], [1, 0]], np.float32)
    a = tr.texture_stage(s, nrm, faces, fid, vt, faces, lv, SHADE, LIGHTS, 0.01, BG)
    # the winding of a face does not move its texture: corners 1 and 2 are swapped together with the vertices
    b = tr.texture_stage(s, nrm, faces[:, [0, 2, 1]], fid, vt, faces[:, [0, 2, 1]], lv, SHADE, LIGHTS, 0.01, BG)
    assert np.allclose(a["u"], b["u"], atol=1e-15) and np.allclose(a["v"], b["v"], atol=1e-15)
    j = (np.arange(n) + 0.5) / n
    assert np.abs(a["u"] - j[None, :]).max() < 1e-12 and np.abs(a["v"] - (1 - j)[:, None]).max() < 1e-12
    # flat, camera-facing, five lights of intensity 2: (T / 255)(0.2 + 10 / pi) clamps to 1 for 128 and 255, not for 64
    k = 64 / 255 * (float(np.float32(0.2)) + 10 * float(np.float32(0.318309886183790672)))   # the fp32 constants
    assert np.abs(a["color"][..., 0] - k).max() < 1e-12 and (a["color"][..., 1:] == 1.0).all()
    assert (a["color_u8"] == np.array([np.floor(255 * k + 0.5), 255, 255])).all()
    # an index outside vt counts as (0, 0); pixels outside the mesh keep zeros and the background colour
    bad = faces.copy()
    bad[0, 0] = 99
    c = tr.texture_stage(s, nrm, faces, fid, vt, bad, lv, SHADE, LIGHTS, 0.01, BG)
    z = tr.texture_stage(s, nrm, faces, fid, np.array([[0, 0], [1, 1], [0, 0], [1, 0]], np.float32), faces, lv, SHADE, LIGHTS, 0.01, BG)
    assert np.array_equal(c["v"][fid == 0], z["v"][fid == 0]) and np.array_equal(c["v"][fid == 1], a["v"][fid == 1])
    fid2 = fid.copy()
    fid2[0, :] = -1
    d = tr.texture_stage(s, nrm, faces, fid2, vt, faces, lv, SHADE, LIGHTS, 0.01, BG)
    assert (d["u"][0] == 0).all() and (d["lam"][0] == 0).all() and (d["color_u8"][0] == 255).all() and (d["color"][0] == 1.0).all()


def test_validator_errors():
    from msmd_amd.utils.renderer import validate_texture
    img = _img(5, 3)
    vt = np.array([[0, 0], [1, 0], [0, 1], [1, 1]], np.float64)
    ft = np.array([[0, 1, 2], [1, 3, 2]], np.int64)
    i, v, f = validate_texture(img, {"vt": vt, "ft": ft}, 2)
    assert i.dtype == np.uint8 and v.dtype == np.float32 and f.dtype == np.int32 and v.shape == (4, 2) and f.shape == (2, 3)
    assert all(a.flags["C_CONTIGUOUS"] for a in (i, v, f))
    validate_texture(_img(2, 2, 0, 4), {"vt": vt.astype(np.float32), "ft": ft.astype(np.uint16)}, 2)
    for bad_ft in (ft + 2, ft - 1, ft[:1], np.concatenate([ft, ft])):
        with pytest.raises(ValueError):
            validate_texture(img, {"vt": vt, "ft": bad_ft}, 2)
    with pytest.raises(ValueError):
        validate_texture(np.zeros((4097, 1, 3), np.uint8), {"vt": vt, "ft": ft}, 2)
    with pytest.raises(ValueError):
        validate_texture(np.zeros((0, 4, 3), np.uint8), {"vt": vt, "ft": ft}, 2)
    for bad_img in (img.astype(np.float32), img.astype(np.int32), img[..., 0], img[..., :2], img[None]):
        with pytest.raises(TypeError):
            validate_texture(bad_img, {"vt": vt, "ft": ft}, 2)
    for bad_uv in ({"vt": vt.astype(np.int32), "ft": ft}, {"vt": vt, "ft": ft.astype(np.float32)}, {"vt": vt[:, :1], "ft": ft},
                   {"vt": vt.ravel(), "ft": ft}, {"vt": vt, "ft": ft[:, :2]}, {"vt": vt}, None, (vt, ft)):
        with pytest.raises(TypeError):
            validate_texture(img, bad_uv, 2)


def test_renderer_refuses_a_texture_without_a_table_and_takes_the_keywords():
    import inspect
    from msmd_amd import inference
    from msmd_amd.utils.renderer import MeshRenderer
    r = MeshRenderer((8, 8))
    mesh = type("M", (), {"v": np.zeros((3, 3)), "f": np.array([[0, 1, 2]])})()
    with pytest.raises(NotImplementedError, match="uv table"):
        r.render_mesh(mesh, np.zeros(3), tex_img=np.zeros((4, 4, 3), np.uint8))
    p = inspect.signature(MeshRenderer.render_vertices).parameters
    assert all(p[k].default is d for k, d in (("tex_img", None), ("tex_uv", None), ("return_uv", False)))
    for fn in (inference.render_coeffs, inference.render_coeffs_chunks):
        p = inspect.signature(fn).parameters
        assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY and p[k].default is None for k in ("tex_img", "tex_uv"))


def test_parse_args_texture(tmp_path, capsys):
    from msmd_amd.inference import load_texture, parse_args
    req = ["--model_root", "r", "--model_name", "n", "--model_iter", "1", "--style_clip_exp_code_path", "e",
           "--style_clip_head_rot_path", "h", "--audio_clip", "a"]
    assert parse_args(req).texture is None
    a = parse_args(req + ["--texture", "t.npz", "--render_size", "64"])
    assert a.texture == "t.npz" and not a.video
    a = parse_args(req + ["--texture", "t.npz", "--render_size", "64", "--video"])
    assert a.texture == "t.npz" and a.video
    for extra in (["--texture", "t.npz"], ["--texture", "t.npz", "--render_size", "0"]):
        with pytest.raises(SystemExit):
            parse_args(req + extra)
        assert "--texture needs --render_size" in capsys.readouterr().err
    path = str(tmp_path / "t.npz")
    img, vt, ft = _img(4, 4), np.zeros((3, 2), np.float32), np.array([[0, 1, 2]], np.int32)
    np.savez(path, tex_img=img, vt=vt, ft=ft)
    got, uv = load_texture(path)
    assert np.array_equal(got, img) and np.array_equal(uv["vt"], vt) and np.array_equal(uv["ft"], ft)
    np.savez(path, tex_img=img, vt=vt)
    with pytest.raises(ValueError):
        load_texture(path)


def test_sphere_cases_reach_the_levels_the_gpu_test_asserts():
    """The 7 x 16 sphere at 64 x 64: lambda > 1 on at least half its pixels under the 256^2 texture, lambda = 0 on at least half
    under the 8^2 one (its centre sees about 3.6 texels per pixel vertically at 256^2, about 0.11 at 8^2)."""
    from msmd_amd import synth
    from msmd_amd.utils.renderer import MeshRenderer
    v, f = synth.latlong_sphere(7, 16, 0.09)
    vt, ft = tr.sphere_uv(7, 16)
    assert vt.shape[0] > v.shape[0] and ft.shape == f.shape and ft.max() == vt.shape[0] - 1
    r = MeshRenderer((64, 64))
    view = np.linalg.inv(r.camera_pose)[:3].astype(np.float32)
    screen, normals = rr.vertex_stage(v[None], f, view, np.float32(1.0 / np.tan(r.fov / 2.0)), 64, 64, dtype=np.float32)
    fid = rr.raster_stage(screen[0], normals[0], f, 64, 64, 0.01, 3.0, SHADE, LIGHTS, BG)["face_id"]
    covered = fid >= 0
    assert covered.sum() > 1000
    for side, cond in ((256, lambda lam: lam > 1), (8, lambda lam: lam == 0)):
        lv = tr.pyramid(tr.noise_texture(f"texture/noise{side}", side, side))
        out = tr.texture_stage(screen[0], normals[0], f, fid, vt, ft, lv, SHADE, LIGHTS, 0.01, BG)
        share = cond(out["lam"][covered]).mean()
        print(f"{side}^2: condition holds on {100 * share:.1f} % of {int(covered.sum())} pixels; "
              f"lambda at the centre {out['lam'][32, 32]:.3f}")
        assert share >= 0.5
        # the seam column: u stays within [0, 1] and is monotone in the face, never interpolated from 15/16 back to 0
        assert out["u"][covered].min() >= 0 and out["u"][covered].max() <= 1
