"""Face crops without a GPU: the host side of msmd_amd.utils.face_crop against the reference's recorded outputs
(tests/golden/g16_face_crop.npz: box tracker, box smoothing, crop_img / get_affine_transform), self-checks of the float64
restatement of the warp (tests/crop_ref.py), the C header and the built library's export and argument checks."""
import ctypes
import json

import numpy as np
import pytest
import torch

import crop_ref as CR
from conftest import load_golden

MODES = ("", "savgol", "savgol_center_and_constant_size")


@pytest.fixture(scope="module")
def g():
    return load_golden("g16_face_crop")


def frames_of(g, name):
    frames = [[] for _ in range(int(g[f"track/{name}/n_frames"]))]
    for f, fid, x, y, w, h in g[f"track/{name}/detections"].tolist():
        frames[f].append((fid, (x, y, w, h)))
    return frames


def test_archive_holds_the_listed_cases(g):
    want = {"one_face", "gap1", "first_missing", "last_missing", "two_faces_mid_above", "two_faces_mid_below", "two_faces_early",
            "first_two_ahead0", "first_two_ahead1", "first_two_ahead3"}
    assert {str(c) for c in g["track/cases"]} == want
    assert str(g["track/gap2_note"]).startswith("ValueError") and json.loads(str(g["versions"]))["numpy"] == "2.2.6"
    assert [int(F) for F in g["smooth/lengths"]] == [5, 6, 40]
    assert set(g["tf/boxes"][:, 1].tolist()) >= {2, 3, 200, 1079} and g["tf/sizes"].tolist() == [224, 256]
    # scipy does not return a constant track: the note the snap rule of smooth_boxes rests on
    c_in, c_out = g["smooth/constant_in"], g["smooth/constant_scipy"]
    assert (c_out != c_in).any() and np.abs(c_out - c_in).max() < 1e-9 and (c_out.astype(np.int32) != c_in.astype(np.int32)).any()


def test_track_boxes_equals_the_reference_exactly(g):
    from msmd_amd.utils.face_crop import track_boxes
    for name in (str(c) for c in g["track/cases"]):
        boxes, flag = track_boxes(frames_of(g, name), 5)
        assert boxes.dtype == np.float64 and np.array_equal(boxes, g[f"track/{name}/boxes"]), name
        assert flag == json.loads(str(g[f"track/{name}/flags"])), name
    # the quirks, by name: two earlier frames never reach 0.4 after the division by K; the below-threshold frame repeats
    assert np.array_equal(g["track/two_faces_early/boxes"][2], g["track/two_faces_early/boxes"][1])
    assert np.array_equal(g["track/two_faces_mid_below/boxes"][7], g["track/two_faces_mid_below/boxes"][6])


def test_track_boxes_fills_a_long_gap_from_its_two_ends(g):
    from msmd_amd.utils.face_crop import track_boxes
    frames = frames_of(g, "one_face")
    full = track_boxes(frames)[0]
    holes = [list(f) for f in frames]
    holes[2] = holes[3] = holes[4] = []
    boxes, flag = track_boxes(holes)
    for i in (2, 3, 4):
        line = full[1] + (full[5] - full[1]) * ((i - 1) / 4.0)
        assert np.abs(boxes[i] - line).max() <= 1e-12 * np.abs(line).max()
    assert np.array_equal(boxes[[0, 1, 5, 6, 7]], full[[0, 1, 5, 6, 7]]) and flag["has_missing"] and not flag["no_first_frame"]
    holes[0] = holes[1] = holes[7] = []
    boxes, flag = track_boxes(holes)
    assert np.array_equal(boxes[:5], np.tile(full[5], (5, 1))) and np.array_equal(boxes[7], full[6])
    assert flag["no_first_frame"] and flag["no_last_frame"]
    with pytest.raises(ValueError):
        track_boxes([[], [], []])


@pytest.mark.parametrize("mode", range(3))
def test_smooth_boxes_equals_the_reference_exactly(g, mode):
    from msmd_amd.utils.face_crop import smooth_boxes
    for F in (int(v) for v in g["smooth/lengths"]):
        got = smooth_boxes(g[f"smooth/{F}/boxes"], MODES[mode])
        assert got.dtype == np.int32 and np.array_equal(got, g[f"smooth/{F}/mode{mode}"]), (F, MODES[mode])


def test_smooth_boxes_returns_a_constant_track_and_refuses_short_clips(g):
    from msmd_amd.utils.face_crop import smooth_boxes
    x, y, w, h = g["smooth/constant_in"][0]
    want = np.tile(np.array([[h, w, x + w // 2, y + h // 2]], np.int32), (9, 1))
    assert np.array_equal(smooth_boxes(g["smooth/constant_in"], "savgol"), want)
    assert np.array_equal(smooth_boxes(g["smooth/constant_in"], ""), want)
    for window, polyorder in ((7, 2), (5, 3), (9, 4)):
        assert np.array_equal(smooth_boxes(g["smooth/constant_in"], "savgol", window, polyorder), want)
    wide = smooth_boxes(g["smooth/constant_in"], "savgol_center_and_constant_size", over_crop_ratio=1.5)
    assert np.array_equal(wide[:, :2], np.tile(np.array([[10, 450]], np.int32), (9, 1)))            # 7 * 1.5 truncated, 300 * 1.5
    with pytest.raises(ValueError):
        smooth_boxes(np.zeros((4, 4)) + 50)
    with pytest.raises(ValueError):
        smooth_boxes(np.zeros((9, 4)) + 50, "median")
    assert smooth_boxes(np.zeros((4, 4)) + 50, "").shape == (4, 4)


def test_crop_transforms_against_the_exact_solve(g):
    from msmd_amd.utils.face_crop import crop_transforms
    bound = max(8.0 * float(g["tf/err_lu"].max()), 4.0 * np.finfo(np.float64).eps)
    worst = 0.0
    for si, S in enumerate(g["tf/sizes"].tolist()):
        got, truth = crop_transforms(g["tf/boxes"], S), g["tf/truth"][si]
        assert got.shape == truth.shape and got.dtype == np.float64
        err = np.abs(got - truth).max(-1) / np.abs(truth).max(-1)
        worst = max(worst, float(err.max()))
    print(f"crop_transforms against the exact solve: worst relative error {worst:.3e}; "
          f"np.linalg.solve's err_lu {float(g['tf/err_lu'].max()):.3e}, bound {bound:.3e}")
    assert worst <= bound
    # crop_img's own numbers: centre and scale * 1.15
    b = g["tf/boxes"].astype(np.float64)
    assert np.array_equal(g["tf/center"], b[:, 2:]) and np.array_equal(g["tf/scale"], np.maximum(b[:, 1] - 1, b[:, 0] - 1) / 200.0 * 1.15)
    with pytest.raises(ValueError):
        crop_transforms(np.array([[1, 1, 50, 50]]))
    with pytest.raises(ValueError):
        crop_transforms(g["tf/boxes"], 0)
    with pytest.raises(ValueError):
        crop_transforms(g["tf/boxes"], 1025)


def test_the_box_centre_lands_on_the_crop_centre_and_round_trip(g):
    from msmd_amd.utils.face_crop import crop_to_frame, crop_transforms, frame_to_crop
    boxes = g["tf/boxes"]
    tr = crop_transforms(boxes, 256)
    centre = frame_to_crop(boxes[:, None, 2:].astype(np.float64), tr)
    assert np.abs(centre - 128.0).max() <= 1e-9
    rs = np.random.RandomState(3)
    p = rs.uniform(-200, 2200, (len(boxes), 9, 2))
    back = crop_to_frame(frame_to_crop(p, tr), tr)
    assert np.abs(back - p).max() <= 1e-9 * 1920
    # one transform for all points, a rotated one, and torch
    th = np.deg2rad(30.0)
    rot = np.array([[0.7 * np.cos(th), -0.7 * np.sin(th), 11.5], [0.7 * np.sin(th), 0.7 * np.cos(th), -3.25]])
    q = frame_to_crop(p[0], rot)
    assert np.abs(q - (p[0] @ rot[:, :2].T + rot[:, 2])).max() <= 1e-10
    assert np.abs(crop_to_frame(q, rot) - p[0]).max() <= 1e-9 * 1920
    pt = torch.from_numpy(p)
    assert np.abs(crop_to_frame(frame_to_crop(pt, tr), tr).numpy() - p).max() <= 1e-9 * 1920
    with pytest.raises(ValueError):
        frame_to_crop(p[:3], tr)


def test_restatement_identity_shift_and_ties():
    rs = np.random.RandomState(7)
    frames = rs.randint(0, 256, (2, 9, 11, 3)).astype(np.uint8)
    ident = np.tile(np.array([[1.0, 0, 0], [0, 1.0, 0]]), (2, 1, 1))
    assert np.array_equal(CR.warp(frames, ident, 6, 7, swap_rb=False), frames[:, :6, :7])
    assert np.array_equal(CR.warp(frames, ident, 6, 7, swap_rb=True), frames[:, :6, :7, ::-1])
    # output (i, j) reads source (i + 2, j - 3): a zero border on the left, and below once the rows run out
    shift = np.tile(np.array([[1.0, 0, -3.0], [0, 1.0, 2.0]]), (2, 1, 1))
    got = CR.warp(frames, shift, 9, 11, swap_rb=False)
    want = np.zeros_like(got)
    want[:, :7, 3:] = frames[:, 2:, :8]
    assert np.array_equal(got, want)
    # source = output / 2 on a frame whose horizontal neighbour sums are odd: odd columns sit on exact .5 ties and round up
    frame = np.zeros((1, 4, 8, 3), np.uint8)
    frame[0, :, :, :] = (np.arange(8) * 3 % 2 + 2 * np.arange(8))[None, :, None]       # 0 3 4 7 8 11 12 15: sums 3 7 11 15 ...
    half = np.array([[[0.5, 0, 0], [0, 0.5, 0]]])
    got = CR.warp(frame, half, 1, 14, swap_rb=False)[0, 0, :, 0].astype(int)
    row = frame[0, 0, :, 0].astype(int)
    assert ((row[:-1] + row[1:]) % 2 == 1).all()
    assert np.array_equal(got[0::2], row[:7]) and np.array_equal(got[1::2], (row[:-1] + row[1:] + 1) // 2)
    # wild and non-finite coordinates give zeros
    wild = np.array([[[1e300, 0, 0], [0, 1.0, 0]], [[np.nan, 0, 0], [0, 1.0, np.inf]]])
    with np.errstate(all="ignore"):
        assert not CR.warp(np.concatenate([frame, frame]), wild, 3, 3)[:, :, 1:].any()
    # the normalise is the table
    from msmd_amd.utils.face_crop import IMAGENET_MEAN, IMAGENET_STD, normalise_table
    ramp = np.arange(256, dtype=np.uint8).reshape(1, 16, 16, 1).repeat(3, 3)
    tab = normalise_table()
    assert tab.shape == (3, 256) and tab.dtype == torch.float32
    assert torch.equal(CR.normalise(ramp, IMAGENET_MEAN, IMAGENET_STD).reshape(3, 256), tab)


def test_header_declares_and_the_library_exports_the_entry_point():
    from msmd_amd import _lib, ops
    protos = _lib.parse_header()
    assert len(protos["msmd_face_crop"]) == 16
    assert "#define MSMD_CROP_MAX_SIDE 1024" in open(_lib.HEADER).read() and ops.CROP_MAX_SIDE == 1024
    assert hasattr(_lib.load(), "msmd_face_crop")


def test_entry_point_refuses_bad_arguments_before_any_launch():
    """Every call returns 1 from the argument checks: nothing is launched, so no device is needed, and the pointers that stand
    for device memory are never dereferenced."""
    from msmd_amd import _lib, ops
    lib = _lib.load()
    fake = ctypes.c_void_p(4096)

    def call(frames=fake, fs=37 * 160, rs=160, ps=3, F=2, H=37, W=53, inv=fake, table=fake, oh=16, ow=16, out=fake, dt=ops.F32,
             crop=fake):
        return lib.msmd_face_crop(frames, fs, rs, ps, F, H, W, inv, table, oh, ow, 1, out, dt, crop, None)
    assert call(ow=0) == 1 and call(ow=ops.CROP_MAX_SIDE + 1) == 1 and call(oh=0) == 1 and call(oh=ops.CROP_MAX_SIDE + 1) == 1
    assert call(frames=None) == 1 and call(inv=None) == 1 and call(table=None) == 1
    assert call(out=None, crop=None) == 1
    assert call(F=0) == 1 and call(H=0) == 1 and call(W=0) == 1 and call(W=16385) == 1
    assert call(ps=2) == 1 and call(ps=5) == 1
    assert call(rs=158) == 1 and call(fs=36 * 160) == 1             # a row of 53 pixels is 159 bytes; 37 rows need 36 * 160 + 159
    assert call(dt=ops.F16X2) == 1 and call(dt=99) == 1


def test_wrappers_refuse_cpu_tensors_and_bad_transforms():
    from msmd_amd import ops
    from msmd_amd.utils import face_crop as FC
    frames = torch.zeros(2, 8, 8, 3, dtype=torch.uint8)
    ident = np.tile(np.array([[1.0, 0, 0], [0, 1.0, 0]]), (2, 1, 1))
    with pytest.raises(TypeError):
        FC.crop_faces(frames, ident, 8)
    with pytest.raises(TypeError):
        ops.face_crop(frames, torch.from_numpy(ident), FC.normalise_table(), 8)
    with pytest.raises(TypeError):
        next(FC.crop_clip(frames, np.tile(np.array([[1.0, 1, 6, 6]]), (5, 1)), 8))
    singular = ident.copy()
    singular[1, :, :2] = [[1.0, 2.0], [2.0, 4.0]]
    with pytest.raises(ValueError, match="singular"):
        FC.crop_faces(frames, singular, 8)
    bad = ident.copy()
    bad[0, 0, 2] = np.nan
    with pytest.raises(ValueError):
        FC.crop_faces(frames, bad, 8)
    with pytest.raises(ValueError):
        FC.crop_faces(frames, ident[:, :, :2], 8)
    with pytest.raises(ValueError):
        FC.normalise_table(std=(1.0, 0.0, 1.0))
    with pytest.raises(ValueError):
        next(FC.crop_clip(frames, np.tile(np.array([[1.0, 1, 6, 6]]), (4, 1)), 8))           # F < window
    a = FC.parse_args(["--frames", "f.npy", "--boxes", "b.pickle", "--out", "o.npy"])
    assert (a.size, a.smoothing, a.video, a.fps, a.batch_size) == (256, "savgol", None, None, 32)
    a = FC.parse_args(["--frames", "f.npy", "--boxes", "b.pickle", "--out", "o.npy", "--size", "224", "--smoothing", "", "--video",
                       "v.avi", "--fps", "25"])
    assert (a.size, a.smoothing, a.video, a.fps) == (224, "", "v.avi", 25.0)
