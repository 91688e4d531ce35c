"""The truth of the four-sample renderer (tests/render_msaa_ref.py) pinned on its own, without a GPU: it is
render_ref at the pixel centre, its coverage is exact on shapes whose coverage is known, and its resolve is the stated rule.
The float32 vertex stage of render_ref stands in for the GPU's."""
import numpy as np
import pytest

import render_msaa_ref as mr
import render_ref as rr
from msmd_amd import synth

NEAR, FAR = 0.01, 3.0
WHITE = (255, 255, 255, 255)
SHADE = np.array([0.3, 0.3, 0.3, 0.2, 0.2, 0.2], np.float32)
LIGHTS = np.array([[0.0, 0.0, 1.0, 2.0]] * 5, np.float32)
ONE_LIGHT = np.array([[0.0, 0.0, 1.0, 1.0]], np.float32)       # a flat face towards the camera is then a mid grey, not clamped


def scene(name, W, H):
    """fp32 (screen, normals, faces) of test_render_gpu's case `name`, frame 0, through the float32 vertex stage and the
    renderer's default camera (one unit in front of the origin, 16 degrees)."""
    if name == "a":
        v, f = synth.latlong_sphere(7, 16, 0.09)
    else:
        a = synth.flame_asset()
        v, f = a["v_template"].astype(np.float32), a["f"][:600].astype(np.int32)
    pose = np.eye(4)
    pose[:3, 3] = [0, 0, 1]
    view = np.linalg.inv(pose)[:3].astype(np.float32)
    focal = np.float32(1.0 / np.tan(16 / 180 * np.pi / 2.0))
    screen, normals = rr.vertex_stage(v[None], f, view, focal, H, W, dtype=np.float32)
    return screen[0], normals[0], f


def flat(points, depth=1.0):
    """Screen-space vertices (x, y) in pixels at one depth, facing the camera."""
    p = np.asarray(points, np.float32)
    screen = np.concatenate([p, np.full((p.shape[0], 1), depth, np.float32)], axis=1)
    normals = np.tile(np.array([[0, 0, 1]], np.float32), (p.shape[0], 1))
    return screen, normals


@pytest.mark.parametrize("name,W,H", [("a", 37, 53), ("b", 64, 64)])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_the_centre_sample_is_render_ref_bit_for_bit(name, W, H, dtype):
    screen, normals, f = scene(name, W, H)
    want = rr.raster_stage(screen, normals, f, H, W, NEAR, FAR, SHADE, LIGHTS, WHITE, dtype)
    got = mr.raster_samples(screen, normals, f, H, W, NEAR, FAR, SHADE, LIGHTS, WHITE, mr.CENTRE, dtype)
    assert (want["face_id"] >= 0).any() and (want["count"] > 1).any()
    for key, w in want.items():
        g = got[key][:, :, 0]
        assert g.dtype == w.dtype and g.shape == w.shape, key
        assert np.array_equal(g.view(np.uint8) if g.dtype == np.uint8 else g.view(f"u{g.dtype.itemsize}"),
                              w.view(np.uint8) if w.dtype == np.uint8 else w.view(f"u{w.dtype.itemsize}")), key
    assert np.array_equal(mr.ambiguous({k: v[:, :, 0] for k, v in got.items()}), rr.ambiguous(want))


def test_a_vertical_edge_through_the_pixel_centres_covers_the_two_left_samples():
    W, H = 16, 12
    # a rectangle from x = 2 to x = 10.5, rows 3 .. 8: its right edge runs through the centres of column 10
    screen, normals = flat([[2, 3], [10.5, 3], [10.5, 9], [2, 9]])
    f = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    r = mr.raster_samples(screen, normals, f, H, W, NEAR, FAR, SHADE, ONE_LIGHT, WHITE)
    cov = r["face_id"] >= 0
    xs = np.array([s[0] for s in mr.SAMPLES4])
    assert sorted(xs[[2, 0]]) == [32, 96]
    want = np.zeros(4, bool)
    want[[0, 2]] = True                                       # s0 and s2: x offsets 96 and 32, left of the centre
    assert (cov[3:9, 10] == want).all()
    assert cov[3:9, 2:10].all() and not cov[3:9, 11:].any() and not cov[:3].any() and not cov[9:].any() and not cov[:, :2].any()
    out = mr.resolve(r["color_u8"], cov, WHITE)
    c = r["color_u8"][5, 5, 0].astype(np.int64)               # the face's grey: one depth, one normal, so one colour
    assert (r["color_u8"][cov] == c).all() and c[0] == c[1] == c[2] and 0 < c[0] < 255
    assert (out[3:9, 10, :3] == ((2 * c + 2 * 255 + 2) >> 2)).all() and (out[3:9, 10, 3] == 255).all()
    assert (out[3:9, 2:10, :3] == c).all() and (out[~cov.any(-1)] == 255).all()
    # a transparent background: the stored alpha is the coverage
    clear = mr.resolve(r["color_u8"], cov, (0, 0, 0, 0))
    assert np.array_equal(clear[..., 3], ((255 * cov.sum(-1) + 2) >> 2).astype(np.uint8))
    assert (clear[3:9, 10, 3] == 128).all() and (clear[3:9, 10, :3] == ((2 * c + 2) >> 2)).all()


@pytest.mark.parametrize("flip", [False, True])
def test_a_pixel_aligned_rectangle_covers_every_sample_once(flip):
    W, H = 14, 11
    screen, normals = flat([[3, 2], [11, 2], [11, 9], [3, 9]])
    f = np.array([[0, 2, 1], [0, 3, 2]] if flip else [[0, 1, 2], [0, 2, 3]], np.int32)       # either orientation
    r = mr.raster_samples(screen, normals, f, H, W, NEAR, FAR, SHADE, ONE_LIGHT, WHITE)
    inside = np.zeros((H, W, 4), bool)
    inside[2:9, 3:11] = True
    assert np.array_equal(r["count"], inside.astype(np.int32))                            # the diagonal: 1, never 0 or 2
    # no sample lies on that rectangle's diagonal.  The square (2.25, 2) .. (10.25, 10) has the diagonal y = x - 0.25, which
    # passes through s0 = (j + 0.375, i + 0.125) of every pixel with i = j: there the top-left rule alone decides
    screen, normals = flat([[2.25, 2], [10.25, 2], [10.25, 10], [2.25, 10]])
    r = mr.raster_samples(screen, normals, f, H, W, NEAR, FAR, SHADE, ONE_LIGHT, WHITE)
    on_diagonal = [(i, i, 0) for i in range(2, 10)]                                         # s0 of pixel (i, i): (i + .375, i + .125)
    assert all(r["count"][p] == 1 for p in on_diagonal)
    assert r["count"].max() == 1 and r["count"].sum() == 4 * 64


def test_the_summed_coverage_is_the_snapped_area_within_the_pixels_the_edges_cross():
    """A pixel wholly inside the triangle has all four samples covered and adds exactly its area, 1; a pixel wholly outside adds
    0 to both.  Any other pixel adds a coverage / 4 in [0, 1] against an area in [0, 1], so the two sums differ by at most the
    number of such pixels.  A pixel counts as wholly inside when its four corners are strictly inside every edge, as wholly
    outside when all four corners are strictly outside one edge; whatever is left is counted towards the margin (that includes
    a few pixels beside a vertex that no edge crosses, which only makes the margin honest, not smaller)."""
    W, H = 40, 36
    for k, tri in enumerate(([[3.3, 2.1], [36.7, 9.4], [12.2, 33.8]], [[1.0, 30.0], [20.5, 1.25], [38.0, 34.0]],
                             [[5.0, 5.0], [30.0, 5.5], [6.0, 7.0]])):
        screen, normals = flat(tri)
        f = np.array([[0, 1, 2]], np.int32)
        r = mr.raster_samples(screen, normals, f, H, W, NEAR, FAR, SHADE, ONE_LIGHT, WHITE)
        t = rr.face_table(screen, f, NEAR)
        X, Y = t["X"][0], t["Y"][0]
        area = float(t["area"][0]) / 2.0 / 65536.0
        cy, cx = np.meshgrid(256 * np.arange(H + 1, dtype=np.int64), 256 * np.arange(W + 1, dtype=np.int64), indexing="ij")
        e = [rr._edge(X[a], Y[a], X[b], Y[b], cx, cy) for a, b in ((1, 2), (2, 0), (0, 1))]
        corners = lambda m: np.stack([m[:-1, :-1], m[:-1, 1:], m[1:, :-1], m[1:, 1:]])
        inside = np.all([corners(x > 0).all(0) for x in e], axis=0)
        outside = np.any([corners(x < 0).all(0) for x in e], axis=0)
        margin = int((~inside & ~outside).sum())
        cov = r["count"].sum() / 4.0
        print(f"triangle {k}: snapped area {area:.3f} px, coverage / 4 = {cov:.2f}, margin {margin} px, {int(inside.sum())} pixels inside")
        assert (r["count"][inside] == 1).all() and (r["count"][outside] == 0).all()
        assert abs(cov - area) <= margin and (margin < area or k == 2)      # the third is a sliver: every pixel it meets is crossed


def test_the_sample_table():
    s = np.array(mr.SAMPLES4)
    assert s.shape == (4, 2) and s.dtype.kind == "i"
    assert len(set(s[:, 0])) == 4 and len(set(s[:, 1])) == 4
    assert ((s > 0) & (s < 256)).all()
    assert tuple(s.mean(0)) == (128.0, 128.0)
    assert mr.SAMPLES4 == ((96, 32), (224, 96), (32, 160), (160, 224))
    # the box rule of the set-up follows from the least and the greatest offset: + 31 and - 32
    assert 255 - s.max() == 31 and s.min() == 32
    from msmd_amd import ops
    assert ops.RENDER_SAMPLES == (1, 4)


def test_the_parser_takes_render_samples_with_a_render_size_only():
    from msmd_amd.inference import parse_args
    req = ["--model_root", "r", "--model_name", "n", "--model_iter", "1", "--style_clip_exp_code_path", "e",
           "--style_clip_head_rot_path", "h", "--audio_clip", "a.wav"]
    assert parse_args(req).render_samples == 1
    assert parse_args(req + ["--render_size", "64"]).render_samples == 1
    assert parse_args(req + ["--render_size", "256", "--render_samples", "4", "--video"]).render_samples == 4
    assert parse_args(req + ["--render_samples", "1"]).render_samples == 1
    for bad in (["--render_samples", "4"], ["--render_samples", "4", "--render_size", "0"]):
        with pytest.raises(SystemExit):
            parse_args(req + bad)


@pytest.mark.parametrize("n", ["3", "2", "0", "8", "four"])
def test_the_parser_refuses_other_sample_counts(n):
    from msmd_amd.inference import parse_args
    req = ["--model_root", "r", "--model_name", "n", "--model_iter", "1", "--style_clip_exp_code_path", "e",
           "--style_clip_head_rot_path", "h", "--audio_clip", "a.wav"]
    assert parse_args(req + ["--render_size", "64", "--render_samples", "4"]).render_samples == 4
    with pytest.raises(SystemExit):
        parse_args(req + ["--render_size", "64", "--render_samples", n])


def test_the_renderer_takes_one_or_four_samples():
    import inspect
    from msmd_amd.utils.renderer import MeshRenderer
    names = list(inspect.signature(MeshRenderer.__init__).parameters)
    assert names[-1] == "samples" and inspect.signature(MeshRenderer.__init__).parameters["samples"].default == 1
    assert MeshRenderer((8, 8)).samples == 1 and MeshRenderer((8, 8), samples=4).samples == 4
    for bad in (0, 2, 3, 8, "4", None):
        with pytest.raises(ValueError):
            MeshRenderer((8, 8), samples=bad)
