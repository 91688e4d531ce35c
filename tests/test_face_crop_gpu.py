"""msmd_face_crop on the device against the float64 restatement of its operator (tests/crop_ref.py): the uint8
crop byte for byte, the fp32 output as the table lookup, bf16 / fp16 as its rounding; every remainder of the four-pixel lane,
frames whose rows are never 16-byte aligned, pitched and RGBA layouts, batches against single frames, guard bands around both
outputs, and the chain from detections to crops with its command line."""
import io
import pickle

import numpy as np
import pytest
import torch

import crop_ref as CR
import jpeg_ref as jr

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = {"37x53": (37, 53), "64x48": (64, 48)}
SIZES = (1, 4, 5, 16, 17, 33)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def make_frames(F, H, W, C=3, seed=0):
    """Noise over a gradient: neighbours differ, so a wrong weight or neighbour changes bytes."""
    rs = np.random.RandomState(1000 * seed + H + W + C)
    y, x = np.mgrid[0:H, 0:W]
    base = (3 * x + 5 * y)[None, :, :, None] + 40 * np.arange(C)[None, None, None, :] + 17 * np.arange(F)[:, None, None, None]
    return ((base + rs.randint(0, 120, (F, H, W, C))) % 256).astype(np.uint8)


def transform_cases(H, W, S):
    """name -> forward (2, 3) map, frame -> crop."""
    from msmd_amd.utils.face_crop import crop_transforms
    A = lambda a, b, c, d, e, f: np.array([[a, b, c], [d, e, f]], np.float64)
    th = np.deg2rad(30.0)
    c, s = 0.8 * np.cos(th), 0.8 * np.sin(th)
    cases = {
        "identity": A(1, 0, 0, 0, 1, 0),
        "shift_in": A(1, 0, -3, 0, 1, -2),                        # output (i, j) reads source (i + 2, j + 3)
        "shift_out": A(1, 0, 5, 0, 1, -4),                        # ... (i + 4, j - 5): a zero border on the left
        "scale2": A(2, 0, 0, 0, 2, 0),                            # source = output / 2: exact .5 ties
        "scale_half": A(0.5, 0, 0, 0, 0.5, 0),
        "last_column_row": A(1, 0, -(W - S), 0, 1, -(H - S)),     # output S - 1 reads source W - 1, H - 1 exactly
        "minus_half": A(1, 0, 0.5, 0, 1, 0.25),                   # sources in (-1, 0) at the first column and row
        "rotated": A(c, -s, S / 2 - (c * W / 2 - s * H / 2), s, c, S / 2 - (s * W / 2 + c * H / 2)),
    }
    boxes = {"over_left": (20, 18, 2, H // 2), "over_right": (18, 21, W - 2, H // 2), "over_top": (21, 21, W // 2, 1),
             "over_bottom": (17, 20, W // 2, H - 1), "over_corner": (20, 20, W, H), "outside": (20, 20, -200, H // 2)}
    for name, box in boxes.items():
        cases[name] = crop_transforms(np.array([box], np.int32), S)[0]
    return cases


def expected(frames_np, trans, S, swap_rb=True):
    crop = CR.warp(frames_np, CR.invert(trans), S, S, swap_rb)
    return crop, CR.normalise(crop, MEAN, STD)


def check_the_cases(names, want_u8, frames_np, S):
    """What each case is there for, read off the restatement's output."""
    H, W = frames_np.shape[1:3]
    of = lambda name: (want_u8[names.index(name)], frames_np[names.index(name)])
    assert not of("outside")[0].any()
    crop, frame = of("identity")
    assert np.array_equal(crop, frame[:S, :S, ::-1])
    crop, frame = of("last_column_row")
    assert np.array_equal(crop[S - 1, S - 1], frame[H - 1, W - 1, ::-1])
    assert not of("shift_out")[0][:, :min(5, S)].any()
    if S >= 16:
        for name in ("over_left", "over_right", "over_top", "over_bottom", "over_corner"):
            lit = of(name)[0].reshape(-1, 3).max(1) > 0
            assert lit.any() and not lit.all(), name
        assert of("rotated")[0].any() and of("minus_half")[0][0, 0].any()


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16 if t.element_size() == 2 else t.dtype).numpy()


@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_every_transform_case_equals_the_restatement(shape, S):
    from msmd_amd.utils.face_crop import crop_faces, normalise_table
    H, W = SHAPES[shape]
    cases = transform_cases(H, W, S)
    trans = np.stack(list(cases.values()))
    frames_np = make_frames(len(cases), H, W)
    frames = torch.from_numpy(frames_np).to(DEV)
    want_u8, want_f32 = expected(frames_np, trans, S)
    out, crop = crop_faces(frames, trans, S, return_uint8=True)
    assert out.shape == (len(cases), 3, S, S) and out.dtype == torch.float32 and crop.shape == (len(cases), S, S, 3)
    got = crop.cpu().numpy()
    for k, name in enumerate(cases):
        assert np.array_equal(got[k], want_u8[k]), (name, int(np.abs(got[k].astype(int) - want_u8[k]).max()))
    tab = normalise_table()
    lookup = torch.stack([tab[c][torch.from_numpy(want_u8[..., c].astype(np.int64))] for c in range(3)], 1)
    assert torch.equal(lookup, want_f32)                                          # the table is torch's own expression
    assert np.array_equal(bits(out), bits(want_f32))
    for dtype in (torch.bfloat16, torch.float16):
        low = crop_faces(frames, trans, S, dtype=dtype)
        assert low.dtype == dtype and np.array_equal(bits(low), bits(want_f32.to(dtype)))
    # what the cases are there for
    names = list(cases)
    check_the_cases(list(cases), want_u8, frames_np, S)
    black = ((torch.zeros(3) - torch.tensor(MEAN)) / torch.tensor(STD)).view(3, 1, 1).expand(3, S, S)
    assert torch.equal(out[list(cases).index("outside")].cpu(), black)


@pytest.mark.parametrize("layout", ["pitched", "rgba", "rgba_view", "no_swap"])
@pytest.mark.parametrize("F", [1, 3, 7])
def test_input_layouts_and_batch_sizes(F, layout):
    from msmd_amd.utils.face_crop import crop_faces
    H, W, S = 37, 53, 17
    cases = transform_cases(H, W, S)
    trans = np.stack([cases[n] for n in ("rotated", "over_corner", "minus_half", "scale2", "over_left", "last_column_row",
                                         "scale_half")][:F])
    C = 3 if layout in ("pitched", "no_swap") else 4
    frames_np = make_frames(F, H, W, C, seed=F)
    if layout == "pitched":
        wide = torch.full((F, H, W + 5, 3), 255, dtype=torch.uint8, device=DEV)
        wide[:, :, :W] = torch.from_numpy(frames_np).to(DEV)
        frames = wide[:, :, :W]
        assert frames.stride(1) == (W + 5) * 3 and not frames.is_contiguous()
    elif layout == "rgba_view":
        frames = torch.from_numpy(frames_np).to(DEV)[..., :3]
        assert frames.stride(2) == 4
    else:
        frames = torch.from_numpy(frames_np).to(DEV)
    swap = layout != "no_swap"
    want_u8, want_f32 = expected(frames_np, trans, S, swap)
    out, crop = crop_faces(frames, trans, S, swap_rb=swap, return_uint8=True)
    assert np.array_equal(crop.cpu().numpy(), want_u8) and np.array_equal(bits(out), bits(want_f32))


def test_a_frame_does_not_depend_on_its_batch():
    from msmd_amd.utils.face_crop import crop_faces
    H, W, S, F = 64, 48, 33, 7
    cases = transform_cases(H, W, S)
    trans = np.stack([cases[n] for n in ("rotated", "over_corner", "minus_half", "scale2", "over_left", "identity", "scale_half")])
    frames = torch.from_numpy(make_frames(F, H, W, seed=5)).to(DEV)
    out, crop = crop_faces(frames, trans, S, dtype=torch.bfloat16, return_uint8=True)
    again, crop2 = crop_faces(frames, trans, S, dtype=torch.bfloat16, return_uint8=True)
    assert torch.equal(out, again) and torch.equal(crop, crop2)
    rev, crop_r = crop_faces(frames.flip(0), trans[::-1].copy(), S, dtype=torch.bfloat16, return_uint8=True)
    assert torch.equal(rev.flip(0), out) and torch.equal(crop_r.flip(0), crop)
    for f in range(F):
        one, crop1 = crop_faces(frames[f:f + 1], trans[f:f + 1], S, dtype=torch.bfloat16, return_uint8=True)
        assert torch.equal(one[0], out[f]) and torch.equal(crop1[0], crop[f])


@pytest.mark.parametrize("S, lead", [(16, 64), (16, 3), (17, 64), (4, 1)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_entry_point_writes_exactly_its_buffers(dtype, S, lead):
    """Both outputs sit inside marked buffers, `lead` elements in: 64 keeps them aligned for the wide stores where S allows
    them, 3 and 1 do not, and the bits are the same."""
    from msmd_amd import _lib, ops
    from msmd_amd.utils.face_crop import invert_transforms, normalise_table
    H, W, F = 37, 53, 3
    cases = transform_cases(H, W, S)
    trans = np.stack([cases[n] for n in ("rotated", "over_corner", "scale2")])
    frames_np = make_frames(F, H, W, seed=9)
    want_u8, want_f32 = expected(frames_np, trans, S)
    frames = torch.from_numpy(frames_np).to(DEV)
    inv = torch.from_numpy(invert_transforms(trans)).to(DEV)
    tab = normalise_table().to(DEV)
    n_out, n_crop, tail = F * 3 * S * S, F * S * S * 3, 64
    mark = 7.0
    out = torch.full((lead + n_out + tail,), mark, device=DEV, dtype=dtype)
    crop = torch.full((lead + n_crop + tail,), 77, device=DEV, dtype=torch.uint8)
    code = {torch.float32: ops.F32, torch.bfloat16: ops.BF16}[dtype]
    st = torch.cuda.current_stream().cuda_stream
    rc = _lib.load().msmd_face_crop(frames.data_ptr(), H * W * 3, W * 3, 3, F, H, W, inv.data_ptr(), tab.data_ptr(), S, S, 1,
                                    out[lead:].data_ptr(), code, crop[lead:].data_ptr(), st)
    torch.cuda.synchronize()
    assert rc == 0
    assert bool((out[:lead] == mark).all()) and bool((out[lead + n_out:] == mark).all())
    assert bool((crop[:lead] == 77).all()) and bool((crop[lead + n_crop:] == 77).all())
    assert np.array_equal(crop[lead:lead + n_crop].view(F, S, S, 3).cpu().numpy(), want_u8)
    assert np.array_equal(bits(out[lead:lead + n_out].view(F, 3, S, S)), bits(want_f32.to(dtype)))
    # one output at a time
    only = torch.full((n_out + tail,), mark, device=DEV, dtype=dtype)
    assert _lib.load().msmd_face_crop(frames.data_ptr(), H * W * 3, W * 3, 3, F, H, W, inv.data_ptr(), tab.data_ptr(), S, S, 1,
                                      only.data_ptr(), code, None, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(only[:n_out], out[lead:lead + n_out]) and bool((only[n_out:] == mark).all())


def clip_with_a_square(F=12, H=96, W=128):
    """A bright square that drifts, the box a detector would put around it, a second face in two frames and one frame
    without a detection."""
    frames = np.zeros((F, H, W, 3), np.uint8)
    raw, squares = [], []
    for f in range(F):
        x, y, w, h = 40 + 2 * f, 25 + f, 44, 46
        sq = (x + 12, y + 13, 20, 20)
        frames[f, sq[1]:sq[1] + sq[3], sq[0]:sq[0] + sq[2]] = (250, 200, 150)
        squares.append(sq)
        dets = [(0, (x, y, w, h))]
        if f in (7, 8):
            dets.insert(0, (1, (2, 3, 30, 30)))
        raw.append([] if f == 4 else dets)
    return frames, raw, squares


def test_detections_to_crops_end_to_end():
    from msmd_amd.utils.face_crop import crop_faces, crop_transforms, frame_to_crop, smooth_boxes, track_boxes
    S = 33
    frames_np, raw, squares = clip_with_a_square()
    boxes, flag = track_boxes(raw)
    assert flag["has_missing"] and flag["has_multiple"] and (boxes[:, 0] >= 40).all()          # the second face is never taken
    trans = crop_transforms(smooth_boxes(boxes), S)
    out, crop = crop_faces(torch.from_numpy(frames_np).to(DEV), trans, S, return_uint8=True)
    assert np.array_equal(crop.cpu().numpy(), CR.warp(frames_np, CR.invert(trans), S, S))
    crop = crop.cpu().numpy()
    for f, (x, y, w, h) in enumerate(squares):
        corners = frame_to_crop(np.array([[x, y], [x + w - 1, y + h - 1]], np.float64), trans[f])
        bright = crop[f, :, :, 2] >= 125                         # the square's red (250) arrives in channel 2
        rows, cols = np.flatnonzero(bright.any(1)), np.flatnonzero(bright.any(0))
        edges = np.array([[cols[0], rows[0]], [cols[-1], rows[-1]]], np.float64)
        assert np.abs(edges - corners).max() <= 1.0, (f, edges, corners)
        assert 0 < corners.min() and corners.max() < S - 1


def test_command_line_writes_the_crops_and_a_video(tmp_path):
    from PIL import Image
    from msmd_amd.utils import face_crop as FC
    S = 17
    frames_np, raw, _ = clip_with_a_square()
    np.save(tmp_path / "clip.npy", frames_np)
    with open(tmp_path / "clip.pickle", "wb") as f:
        pickle.dump({"raw_bbox_frames": raw, "fps": 25}, f)
    FC.main(["--frames", str(tmp_path / "clip.npy"), "--boxes", str(tmp_path / "clip.pickle"), "--out", str(tmp_path / "crops.npy"),
             "--size", str(S), "--batch_size", "5", "--video", str(tmp_path / "crops.avi")])
    frames = torch.from_numpy(frames_np).to(DEV)
    batches = list(FC.crop_clip(frames, raw, S, batch_size=5))
    assert [b.shape[0] for b, _ in batches] == [5, 5, 2] and all(t.shape == (b.shape[0], 2, 3) for b, t in batches)
    want = torch.cat([b for b, _ in batches]).cpu().numpy()
    got = np.load(tmp_path / "crops.npy")
    assert got.dtype == np.float32 and got.shape == (12, 3, S, S) and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    whole = FC.crop_faces(frames, FC.clip_transforms(raw, S), S)
    assert np.array_equal(bits(whole), want.view(np.int32))
    # the processed boxes of Step 1's pickle are taken before the raw ones
    boxes = FC.track_boxes(raw)[0]
    with open(tmp_path / "clip2.pickle", "wb") as f:
        pickle.dump({"raw_bbox_frames": [[]] * 12, "processed_bbox_frames": [tuple(b) for b in boxes]}, f)
    FC.main(["--frames", str(tmp_path / "clip.npy"), "--boxes", str(tmp_path / "clip2.pickle"), "--out", str(tmp_path / "crops2.npy"),
             "--size", str(S)])
    assert np.array_equal(np.load(tmp_path / "crops2.npy").view(np.uint32), want.view(np.uint32))
    avi = jr.parse_avi((tmp_path / "crops.avi").read_bytes())
    assert len(avi["frames"]) == 12 and avi["streams"][0]["rect"] == (0, 0, S, S) and avi["streams"][0]["rate"] == 25
    for blob in avi["frames"]:
        im = Image.open(io.BytesIO(blob))
        im.load()
        assert im.size == (S, S) and im.mode == "RGB"
    # the video is in the frames' channel order: the square is red-ish in the middle of the crop
    mid = np.asarray(Image.open(io.BytesIO(avi["frames"][0])).convert("RGB"))[S // 2, S // 2].astype(int)
    assert mid[0] > mid[1] > mid[2]
