"""The renderer's numpy truth (tests/render_ref.py) pinned by closed forms, and the renderer's host-side code that needs no
GPU: the vertex -> face table, the constructor's defaults, the command line."""
import numpy as np
import pytest

import render_ref as rr

SHADE = np.array([0.3, 0.3, 0.3, 0.2, 0.2, 0.2], np.float32)
LIGHTS = np.array([[0, 0, 1, 2.0]] * 5, np.float32)
BG = (255, 255, 255)


def _flat(points, depth=1.0):
    """screen rows (x_s, y_s, d) and normals facing the camera for vertices given in pixel coordinates."""
    s = np.array([[x, y, depth] for x, y in points], np.float32)
    return s, np.tile(np.array([[0, 0, 1]], np.float32), (s.shape[0], 1))


def _raster(screen, normals, faces, H, W, **kw):
    return rr.raster_stage(screen, normals, np.asarray(faces), H, W, 0.01, 3.0, SHADE, LIGHTS, BG, **kw)


def test_right_triangle_covers_the_centres_counted_by_hand():
    # legs on the pixel grid lines x = 0 and y = 0, hypotenuse x + y = 4 through the centres with i + j = 3; its oriented
    # vector is (-4, +4): dy > 0, so those centres belong to this triangle -> the 10 pixels with i + j <= 3
    s, n = _flat([(0, 0), (4, 0), (0, 4), (4, 4)])
    i, j = np.mgrid[0:6, 0:6]
    for tri in ([0, 1, 2], [0, 2, 1], [2, 0, 1]):
        r = _raster(s, n, [tri], 6, 6)
        assert np.array_equal(r["face_id"] >= 0, i + j <= 3), tri
        assert r["count"].sum() == 10
    # the triangle on the other side of the hypotenuse gets none of them: every centre on the shared edge is covered once
    for other in ([1, 3, 2], [1, 2, 3]):
        r = _raster(s, n, [[0, 1, 2], other], 6, 6)
        assert np.array_equal(r["count"], ((i < 4) & (j < 4)).astype(np.int32))
        assert np.array_equal(r["face_id"], np.where(i + j <= 3, 0, np.where((i < 4) & (j < 4), 1, -1)))
        alone = _raster(s, n, [other], 6, 6)
        assert np.array_equal(alone["face_id"] >= 0, (i + j > 3) & (i < 4) & (j < 4))
    # without the rule the four centres on the edge are covered twice
    r = _raster(s, n, [[0, 1, 2], [1, 3, 2]], 6, 6, fill_rule=False)
    assert int((r["count"] == 2).sum()) == 4
    # background: colour exactly the background's, depth exactly 0
    assert (r["color_u8"][5, 5] == 255).all() and r["depth"][5, 5] == 0.0 and r["depth"][0, 0] == 1.0
    # flat, camera-facing, five lights of intensity 2 along the normal: 0.3 (0.2 + 10 / pi) clamps to 1
    assert (r["color_u8"][0, 0] == 255).all()


def test_nearer_of_two_overlapping_triangles_wins():
    s = np.array([[0, 0, 1.5], [8, 0, 1.5], [0, 8, 1.5], [0, 0, 1.0], [6, 0, 1.0], [0, 6, 2.0]], np.float32)
    n = np.tile(np.array([[0, 0, 1]], np.float32), (6, 1))
    r = _raster(s, n, [[0, 1, 2], [3, 4, 5]], 8, 8)
    both = r["count"] == 2
    assert both.any()
    # face 1's depth runs from 1 at y = 0 to 2 at y = 6, perspective-correct: 1 / d is linear in screen space
    i, j = np.nonzero(both)
    d_tilted = 1.0 / (1.0 - 0.5 * (i + 0.5) / 6.0)
    assert np.array_equal(r["face_id"][both], np.where(d_tilted < 1.5, 1, 0))
    assert np.allclose(r["depth"][both], np.minimum(d_tilted, 1.5), rtol=1e-12)
    assert np.allclose(r["depth2"][both], np.maximum(d_tilted, 1.5), rtol=1e-12)
    # a face behind `near`, a face with a repeated vertex and a face far off-screen draw nothing
    s2 = np.array([[0, 0, 0.001], [8, 0, 1], [0, 8, 1], [1e7, 1e7, 1]], np.float32)
    r = _raster(s2, n[:4], [[0, 1, 2], [1, 1, 2], [1, 2, 3]], 8, 8)
    assert r["count"].sum() == 0 and (r["face_id"] == -1).all() and (r["depth"] == 0).all()


def test_octahedron_vertex_normals_are_its_normalised_positions():
    v = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64) * 0.37
    f = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]])
    n = rr.vertex_normals(v, f)
    assert np.abs(n - v / np.linalg.norm(v, axis=1, keepdims=True)).max() < 1e-12
    # a vertex in no face gets (0, 0, 1)
    n = rr.vertex_normals(np.concatenate([v, [[5.0, 5, 5]]]), f)
    assert np.array_equal(n[6], [0, 0, 1])
    # the sphere the GPU tests use is wound outwards
    from msmd_amd import synth
    sv, sf = synth.latlong_sphere(7, 16, 0.09)
    assert sv.shape == (114, 3) and sf.shape == (224, 3)
    sn = rr.vertex_normals(sv, sf)
    assert ((sn * sv).sum(1) > 0.08).all()
    bv, bf = synth.latlong_sphere(58, 86, 0.09, n_vertices=synth.FLAME_V)
    assert bv.shape == (synth.FLAME_V, 3) and bf.shape == (synth.FLAME_F, 3)


def test_vertex_stage_projection_closed_form():
    # camera at (0, 0, 1) looking down -z, yfov 90 degrees (focal 1): a point at x = y = 0.5, z = 0 is at depth 1,
    # ndc (0.5, 0.5) -> x_s = 0.75 W, y_s = 0.25 H (row 0 at the top); aspect ratio 1 whatever the image size
    view = np.eye(4)[:3].copy()
    view[2, 3] = -1.0
    v = np.array([[[0.5, 0.5, 0.0], [0.0, 0.0, 0.5], [0.0, 0.0, 0.0]]])
    s, _ = rr.vertex_stage(v, [[0, 1, 2]], view, 1.0, 40, 80)
    assert np.allclose(s[0], [[60.0, 10.0, 1.0], [40.0, 20.0, 0.5], [40.0, 20.0, 1.0]], atol=1e-12)
    # a quarter turn about z around t_center: (0.5, 0.5, 0) - c = (0.5, 0.5, 0) -> (-0.5, 0.5, 0)
    s, n = rr.vertex_stage(v, [[0, 1, 2]], view, 1.0, 40, 80, t_center=np.zeros(3), rot=np.array([[0, 0, np.pi / 2]]))
    assert np.allclose(s[0, 0], [20.0, 10.0, 1.0], atol=1e-5)
    assert np.array_equal(rr.rodrigues(np.zeros(3)), np.eye(3)) and np.allclose(np.linalg.norm(n[0], axis=1), 1.0, atol=1e-12)


def test_vertex_face_table_matches_brute_force():
    from msmd_amd.utils.renderer import vertex_face_csr
    rng = np.random.default_rng(5)
    V, F = 41, 97
    faces = rng.integers(0, V - 1, size=(F, 3))           # vertex V - 1 is in no face
    faces[3] = [7, 7, 9]                                  # a repeated vertex is still one incidence
    off, ids = vertex_face_csr(faces, V)
    assert off.dtype == np.int32 and ids.dtype == np.int32 and off.shape == (V + 1,) and ids.shape == (3 * F,)
    want = rr.csr_brute(faces, V)
    for v in range(V):
        assert ids[off[v]:off[v + 1]].tolist() == want[v], v
    assert off[V] - off[V - 1] == 0 and (ids[off[V]:] == -1).all()
    with pytest.raises(ValueError):
        vertex_face_csr(np.array([[0, 1, V]]), V)


def test_renderer_defaults_without_a_gpu():
    from msmd_amd.utils import renderer as R
    r = R.MeshRenderer((48, 32))
    assert (r.width, r.height) == (48, 32) and r.frustum == {"near": 0.01, "far": 3.0}
    assert np.isclose(r.fov, 16 / 180 * np.pi) and r.bg_color == (255, 255, 255) and R.MeshRenderer((8, 8), black_bg=True).bg_color == (0, 0, 0)
    assert np.array_equal(r.camera_pose[:3, 3], [0, 0, 1]) and np.array_equal(r.camera_pose[:3, :3], np.eye(3))
    assert len(r.light_poses) == 5 and all(np.array_equal(p[:3, :3], np.eye(3)) for p in r.light_poses)
    assert np.allclose(r.light_poses[1][:3, 3], [0, -np.sin(np.pi / 6), np.cos(np.pi / 6)])
    assert np.allclose(R.rodrigues([0.3, -0.2, 0.5]), rr.rodrigues([0.3, -0.2, 0.5]), atol=1e-15)
    mesh = type("M", (), {"v": np.zeros((3, 3)), "f": np.array([[0, 1, 2]])})()
    with pytest.raises(NotImplementedError):
        r.render_mesh(mesh, np.zeros(3), tex_img=np.zeros((4, 4, 3)))
    src = open(R.__file__).read()
    for name in ("pyrender", "trimesh", "cv2", "psbody"):
        assert f"import {name}" not in src and f"from {name}" not in src


def test_parser_keeps_the_reference_defaults_and_adds_rendering_flags():
    from msmd_amd.inference import build_parser
    req = ["--model_root", "r", "--model_name", "n", "--model_iter", "1", "--style_clip_exp_code_path", "e",
           "--style_clip_head_rot_path", "h", "--audio_clip", "a"]
    a = build_parser().parse_args(req)
    assert (a.coef_dict_path, a.cfg_level, a.output_dir, a.versions_of_render) == ("PATH-TO-COEF-STATS", 1.4, "/experiments/refactor", 1)
    assert a.render_size == 0 and a.flame_model_path is None and a.flame_lmk_embedding_path is None
    b = build_parser().parse_args(req + ["--render_size", "256", "--flame_model_path", "m.pkl"])
    assert b.render_size == 256 and b.flame_model_path == "m.pkl"
