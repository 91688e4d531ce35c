"""Per-vertex colours and the error heat map without a GPU: the restatements of tests/vertex_color_ref.py against
the definitions they extend (render_ref.raster_stage), the colour-index rule, the colour tables, the chunk-independence of the error
sums and the command line's refusals."""
import colorsys

import numpy as np
import pytest

import render_ref as rr
import vertex_color_ref as vc
from msmd_amd import synth
from msmd_amd.utils import metrics as M

NEAR, FAR = 0.01, 3.0
WHITE = (255, 255, 255, 255)
SHADE = np.array([0.3, 0.3, 0.3, 0.2, 0.2, 0.2], np.float32)
LIGHTS = np.array([[0.0, 0.0, 1.0, 2.0], [0.0, 0.5, 0.8660254, 2.0], [0.0, -0.5, 0.8660254, 2.0], [0.5, 0.0, 0.8660254, 2.0],
                   [-0.5, 0.0, 0.8660254, 2.0]], np.float32)
# an exactly representable base colour ties the two definitions bit for bit; the others differ from it by the float32 rounding of
# a / 255 that raster_stage's `shade` carries (relative 2^-24), far below what moves a byte except at a tie
COLOURS = [(255, 0, 255), (200, 120, 40), (51, 102, 204)]


def scene(W=48, H=40):
    """The sphere of the GPU tests through render_ref's vertex stage: fp32 screen and normals, the faces, the raster stage's ids."""
    v, f = synth.latlong_sphere(7, 16, 0.09)
    view = np.eye(4)[:3].astype(np.float32).copy()
    view[2, 3] = -1.0                                           # camera at z = 1 looking down -z
    focal = np.float32(1.0 / np.tan(16 / 180 * np.pi / 2.0))
    rot = np.array([[0.3, -0.2, 0.1]], np.float32)
    screen, normals = rr.vertex_stage(v[None], f, view, focal, H, W, t_center=np.zeros(3, np.float32), rot=rot, dtype=np.float32)
    return screen[0].astype(np.float32), normals[0].astype(np.float32), f, W, H


@pytest.mark.parametrize("colour", COLOURS)
def test_constant_colour_lit_is_the_raster_stage_with_that_base_colour(colour):
    screen, normals, f, W, H = scene()
    shade = SHADE.copy()
    shade[:3] = np.asarray(colour, np.float64) / 255.0
    want = rr.raster_stage(screen, normals, f, H, W, NEAR, FAR, shade, LIGHTS, WHITE)
    vcol = np.tile(np.asarray(colour + (7,), np.uint8), (screen.shape[0], 1))
    got = vc.vertex_color_stage(screen, normals, f, want["face_id"], vcol, True, shade, LIGHTS, NEAR, WHITE)
    assert got["covered"].any() and np.array_equal(got["covered"], want["face_id"] >= 0)
    worst = float(np.abs(got["color"] - want["color"]).max())
    print(f"colour {colour}: {int(got['covered'].sum())} covered pixels, worst unquantised difference {worst:.3e}")
    assert np.array_equal(got["color_u8"], want["color_u8"])


@pytest.mark.parametrize("colour", COLOURS)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_constant_colour_unlit_is_that_colour(colour, dtype):
    screen, normals, f, W, H = scene()
    fid = rr.raster_stage(screen, normals, f, H, W, NEAR, FAR, SHADE, LIGHTS, WHITE)["face_id"]
    vcol = np.tile(np.asarray(colour + (0,), np.uint8), (screen.shape[0], 1))
    got = vc.vertex_color_stage(screen, normals, f, fid, vcol, False, SHADE, LIGHTS, NEAR, WHITE, dtype)
    assert got["covered"].any() and (got["color_u8"][got["covered"]] == np.asarray(colour, np.uint8)).all()
    assert (got["color_u8"][~got["covered"]] == 255).all()
    # four samples: every covered sample is that colour, so a fully covered pixel resolves to it
    ids = np.repeat(fid[..., None], 4, axis=-1)
    s4 = vc.vertex_color_samples(screen, normals, f, ids, vcol, False, SHADE, LIGHTS, NEAR, dtype=dtype)
    assert (s4["color_u8"][s4["covered"]] == np.asarray(colour, np.uint8)).all()


def test_three_channel_colours_and_alpha_are_not_read():
    screen, normals, f, W, H = scene()
    fid = rr.raster_stage(screen, normals, f, H, W, NEAR, FAR, SHADE, LIGHTS, WHITE)["face_id"]
    vcol = vc.random_colors("vertex_color/cpu", (screen.shape[0], 4))
    a = vc.vertex_color_stage(screen, normals, f, fid, vcol, True, SHADE, LIGHTS, NEAR, WHITE)
    b = vc.vertex_color_stage(screen, normals, f, fid, vcol[:, :3], True, SHADE, LIGHTS, NEAR, WHITE)
    assert np.array_equal(a["color_u8"], b["color_u8"]) and len(np.unique(a["color_u8"][a["covered"]], axis=0)) > 100


# ------------------------------------------------------------------------------------------------ the colour-index rule
def test_index_rule_of_error_colors():
    lut = np.stack([np.arange(256)] * 4, axis=1).astype(np.uint8)          # row i holds i: the colour IS the index
    lut[:, 3] = 255
    vmax = 0.0125
    step = vmax / 510.0
    # "just under": the rule's own sum t * 255 + 0.5 is rounded to float64, whose spacing below 1 is 2^-53, so the neighbour one ulp
    # under `step` (0.5 - 2^-54 before the addition) rounds to 1.0 by the rule itself; 2^-40 under it the sum is well below 1
    under = step * (1.0 - 2.0 ** -40)
    d = np.array([0.0, vmax, under, step, np.inf, np.nextafter(vmax, 0.0), 2.0 * vmax, 0.5 * vmax])
    got = vc.colormap(d, vmax, lut)[:, 0]
    # t * 255 + 0.5 at t = 1 / 510 is exactly 1 in float64 only if the products round that way: restated from the rule itself
    rule = [255 if x / vmax >= 1.0 else int(np.floor(x / vmax * 255.0 + 0.5)) for x in d]
    print("indices:", got.tolist())
    assert got.tolist() == rule
    assert got[0] == 0 and got[1] == 255 and got[2] == 0 and got[3] == 1 and got[4] == 255 and got[6] == 255 and got[7] == 128
    # through error_colors: a planted distance along x, fp32 and fp16 storage
    for dt in (np.float32, np.float16):
        gt = np.zeros((1, 6, 3), dt)
        pred = gt.copy()
        pred[0, 1, 0] = 1.0
        pred[0, 2, 0] = np.inf
        pred[0, 3] = (np.inf, 0, 0)
        gt[0, 3] = (np.inf, 0, 0)                                          # inf - inf
        pred[0, 4, 1] = np.nan
        pred[0, 5, 2] = 0.25
        c = vc.error_colors(pred, gt, 1.0, lut, (1, 2, 3, 4))
        assert c[0, 0].tolist() == [0, 0, 0, 255] and c[0, 1, 0] == 255 and c[0, 2, 0] == 255
        assert c[0, 3].tolist() == [1, 2, 3, 4] and c[0, 4].tolist() == [1, 2, 3, 4] and c[0, 5, 0] == 64


# ------------------------------------------------------------------------------------------------ colour tables
def test_colormap_tables():
    ends = {"jet": ((0, 0, 255), (255, 0, 0)), "heat": ((0, 0, 0), (255, 255, 255)), "gray": ((0, 0, 0), (255, 255, 255))}
    for name, (lo, hi) in ends.items():
        t = M.colormap_table(name)
        assert t.shape == (256, 4) and t.dtype == np.uint8 and (t[:, 3] == 255).all()
        assert tuple(t[0, :3]) == lo and tuple(t[255, :3]) == hi
    jet = M.colormap_table("jet")
    # the inner stops fall between rows (63.75, 127.5, 191.25): the rows beside them are within one step (4 levels) of the stop
    for row, stop in ((64, (0, 255, 255)), (127, (0, 255, 0)), (128, (0, 255, 0)), (191, (255, 255, 0))):
        assert np.abs(jet[row, :3].astype(np.int64) - np.asarray(stop)).max() <= 4, (row, jet[row])
    hue = np.array([colorsys.rgb_to_hsv(*(c / 255.0))[0] for c in jet[:, :3].astype(np.float64)])
    assert (np.diff(hue) < 0).all() and abs(hue[0] - 2.0 / 3.0) < 1e-12 and hue[-1] == 0.0   # blue down to red, no repeats
    assert (np.abs(np.diff(jet[:, :3].astype(np.int64), axis=0)).sum(1) > 0).all()
    heat = M.colormap_table("heat")
    assert tuple(heat[85, :3]) == (255, 0, 0) and tuple(heat[170, :3]) == (255, 255, 0)
    gray = M.colormap_table("gray")
    assert (gray[:, 0] == np.arange(256)).all() and (gray[:, 1] == gray[:, 0]).all() and (gray[:, 2] == gray[:, 0]).all()
    user = vc.random_colors("vertex_color/user_table", (256, 3))
    padded = M.colormap_table(user)
    assert padded.shape == (256, 4) and np.array_equal(padded[:, :3], user) and (padded[:, 3] == 255).all()
    four = vc.random_colors("vertex_color/user_table4", (256, 4))
    assert np.array_equal(M.colormap_table(four), four)
    for bad in ("viridis", user[:255], user.astype(np.float32), user[:, :2]):
        with pytest.raises(ValueError):
            M.colormap_table(bad)


# ------------------------------------------------------------------------------------------------ error sums
def test_error_sums_do_not_know_the_cuts():
    off, n, V = [0, 1, 6, 8], 8, 5
    g = np.random.default_rng(11)
    pred, gt = g.standard_normal((n, V, 3)).astype(np.float32), g.standard_normal((n, V, 3)).astype(np.float32)
    whole = vc.error_sums(pred, gt, off)
    d = vc.distances(pred, gt)
    for k, (a, b) in enumerate(zip(off[:-1], off[1:])):
        assert np.allclose(whole[k], d[a:b].sum(0), rtol=1e-15, atol=0)
    for chunk in (1, 3, 8):
        cuts = list(range(0, n, chunk)) + [n]
        cut = vc.error_sums(pred, gt, off, cuts)
        assert np.array_equal(cut.view(np.int64), whole.view(np.int64)), chunk
    # a clip's row does not read the other clips, and NaN propagates inside its own
    pred2 = pred.copy()
    pred2[:1] = np.nan
    pred2[6:] = np.nan
    other = vc.error_sums(pred2, gt, off, [0, 3, 6, 8])
    assert np.array_equal(other[1].view(np.int64), whole[1].view(np.int64)) and np.isnan(other[0]).all() and np.isnan(other[2]).all()


# ------------------------------------------------------------------------------------------------ command line
BASE = "--pred_exp a --pred_rot b --gt_exp c --gt_rot d --regions e".split()


@pytest.mark.parametrize("extra", [["--render_size", "64"], ["--error_max", "0.01"], ["--fps", "30", "--error_map", "m.jpg"],
                                   ["--audio", "a.wav", "--error_map", "m.jpg"], ["--error_max", "0", "--error_map", "m.jpg"],
                                   ["--error_max", "-1", "--comparison_video", "v.avi"], ["--error_max", "nan", "--error_map", "m.jpg"],
                                   ["--error_max", "inf", "--error_map", "m.jpg"], ["--render_size", "0", "--error_map", "m.jpg"],
                                   ["--render_samples", "2", "--error_map", "m.jpg"], ["--colormap", "viridis", "--error_map", "m.jpg"],
                                   ["--video_quality", "0", "--comparison_video", "v.avi"], ["--fps", "0", "--comparison_video", "v.avi"]])
def test_parser_refuses(extra, capsys):
    with pytest.raises(SystemExit) as e:
        M.parse_args(BASE + extra)
    assert e.value.code == 2
    assert "error" in capsys.readouterr().err


def test_parser_defaults_and_accepted_combinations():
    a = M.parse_args(BASE)
    assert a.comparison_video is None and a.error_map is None and a.error_max is None and a.render_size == 256 and a.fps == 25.0
    assert a.colormap == "jet" and a.render_samples == 1 and a.audio is None and a.video_quality == 90
    a = M.parse_args(BASE + "--comparison_video v.avi --error_map m.jpg --error_max 0.004 --colormap heat --render_size 64 "
                            "--render_samples 4 --fps 30 --audio a.wav --video_quality 75".split())
    assert (a.comparison_video, a.error_map, a.error_max, a.colormap) == ("v.avi", "m.jpg", 0.004, "heat")
    assert (a.render_size, a.render_samples, a.fps, a.audio, a.video_quality) == (64, 4, 30.0, "a.wav", 75)
    assert M.parse_args(BASE + ["--error_map", "m.jpg", "--render_size", "128"]).render_size == 128


def test_evaluate_coeffs_has_the_callback_and_the_renderer_the_arguments():
    import inspect
    from msmd_amd.utils.renderer import MeshRenderer
    assert inspect.signature(M.evaluate_coeffs).parameters["on_chunk"].default is None
    p = inspect.signature(MeshRenderer.render_vertices).parameters
    assert p["vertex_colors"].default is None and p["lit"].default is True
    assert list(inspect.signature(MeshRenderer.render_mesh).parameters) == ["self", "mesh", "t_center", "rot", "tex_img", "tex_uv",
                                                                           "camera_pose", "light_pose"]
