"""Face crops for an expression encoder: what lies between a decoded video and the expression code in the reference's
dataset_processing/ chain.  Step 1's box tracker (`filter_boxes`) and Step 3's crop front end (box smoothing, `crop_img`'s box
arithmetic, `get_affine_transform`, `crop_v2`'s cv2.warpAffine(INTER_LINEAR), the RGB / BGR swap, ToTensor + Normalize) without
cv2, scipy or torchvision: the box arithmetic runs on the host in numpy float64, the warp and the normalisation on the device,
csrc/face_crop.hip through `ops.face_crop`.

Face detection, video decoding and the encoder itself stay outside: the caller arrives with the frames as a uint8 tensor and
with Step 1's detection lists, and feeds the (N, 3, S, S) batches to their own encoder.  The landmarks an encoder returns in
crop coordinates go back to the frame with `crop_to_frame`, and from there into `utils/head_pose.py`.  The encoder output's own
smoothing ("smooth_expression") is `utils/assemble.py`'s.

Two deviations from the reference, both stated where they are made: `track_boxes` fills a gap of several frames from its two
tracked ends, and `smooth_boxes` counts a smoothed value within 1e-6 below an integer as that integer before it truncates.
The warp is not cv2's fixed-point one.

    python -m msmd_amd.utils.face_crop --frames clip.npy --boxes clip.pickle --out crops.npy [--size 224] [--video crops.avi --fps 25]

`--frames` also takes a Motion-JPEG `.avi` (`utils/media.read_video` decodes it on the device).
"""
from __future__ import annotations

import argparse
import pickle as pkl

import numpy as np
import torch

from .. import ops
from .head_pose import savgol_table

SMOOTHINGS = ("", "savgol", "savgol_center_and_constant_size")
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
SNAP = 1e-6                 # smooth_boxes: a value this close below an integer is that integer


def box_iou(box1, box2):
    """Intersection over union of two (x, y, w, h) boxes; 0 when the union is empty (the reference's calculate_iou)."""
    x1, y1, w1, h1 = box1
    x2, y2, w2, h2 = box2
    inter = max(0, min(x1 + w1, x2 + w2) - max(x1, x2)) * max(0, min(y1 + h1, y2 + h2) - max(y1, y2))
    union = w1 * h1 + w2 * h2 - inter
    return inter / union if union > 0 else 0


def track_boxes(raw_bbox_frames, K=5):
    """One face per frame: Step 1's `filter_boxes` on its own input, a list per frame of (face_id, (x, y, w, h)) (empty where
    nothing was detected) -> (boxes (F, 4) float64 as x, y, w, h; the reference's five flags).

    Its rules, kept as they are.  Frames with detections are numbered among themselves, so "the K frames before" skips empty
    frames.  A frame with one box keeps it.  A frame with several takes the box whose IoU with the kept boxes of the up to K
    frames before, summed and divided by K -- by K also when fewer than K precede, so two earlier frames score 0.4 at most and
    never pass -- is largest, if that exceeds 0.4; otherwise it repeats the previous kept box.  Several boxes in the first
    frame: the one with the largest summed IoU against the first (at most three) single-box frames among the next K.  An
    empty first (last) frame copies the nearest frame that has a box.
    Deviation: an empty frame is the linear interpolation, in float64, of the two nearest frames that have a box.  The
    reference does that for a gap of one frame (and this function returns its numbers there, bit for bit); in a longer gap
    it interpolates from the neighbour it has just filled, which is the same line up to rounding, and under numpy 2 it
    raises instead.  ValueError for a clip without any box."""
    frames = [list(f) for f in raw_bbox_frames]
    flag = dict(has_missing=False, has_multiple=False, no_first_frame=False, no_last_frame=False, multiple_boxes_first_frame=False)
    present = [i for i, f in enumerate(frames) if f]
    if not present:
        raise ValueError("track_boxes: no frame of the clip has a box")
    seen = [frames[i] for i in present]
    kept = []
    for i, boxes in enumerate(seen):
        if len(boxes) == 1:
            kept.append(boxes[0][1])
        elif i == 0:
            flag["multiple_boxes_first_frame"] = flag["has_multiple"] = True
            ahead = [j for j in range(1, min(K + 1, len(seen))) if len(seen[j]) == 1][:3]
            ious = np.zeros(len(boxes))
            for j in ahead:
                ious += np.array([box_iou(b[1], seen[j][0][1]) for b in boxes])
            kept.append(boxes[int(np.argmax(ious))][1])
        else:
            flag["has_multiple"] = True
            ious = np.zeros(len(boxes))
            for j in range(max(0, i - K), i):
                ious += np.array([box_iou(b[1], kept[j]) for b in boxes])
            ious /= K
            kept.append(boxes[int(np.argmax(ious))][1] if np.max(ious) > 0.4 else kept[-1])
    F = len(frames)
    flag["has_missing"] = len(present) < F
    flag["no_first_frame"], flag["no_last_frame"] = present[0] != 0, present[-1] != F - 1
    out = np.empty((F, 4), np.float64)
    out[present] = np.array(kept, np.float64)
    out[:present[0]] = out[present[0]]
    out[present[-1] + 1:] = out[present[-1]]
    for lo, hi in zip(present[:-1], present[1:]):
        if hi - lo > 1:
            slope = (out[hi] - out[lo]) / float(hi - lo)          # scipy's interp1d: slope * (x - x_lo) + y_lo
            for i in range(lo + 1, hi):
                out[i] = slope * float(i - lo) + out[lo]
    return out, flag


def _savgol_apply(x, window, polyorder):
    """scipy.signal.savgol_filter(x, window, polyorder, axis=0, mode='interp') from `savgol_table`'s table, in float64."""
    tab, h, F = savgol_table(window, polyorder), window // 2, x.shape[0]
    edges = tab[window:].reshape(2 * h, window)
    y = np.empty_like(x)
    for j in range(F):
        if j < h:
            y[j] = edges[j] @ x[:window]
        elif j >= F - h:
            y[j] = edges[h + j - (F - h)] @ x[F - window:]
        else:
            y[j] = tab[:window] @ x[j - h:j + h + 1]
    return y


def smooth_boxes(boxes, smoothing="savgol", window=5, polyorder=2, over_crop_ratio=1.2):
    """boxes (F, 4) as x, y, w, h -> int32 (F, 4) as h, w, cx, cy: Step 3's box preparation.  cx = x + w // 2, cy = y + h // 2;
    smoothing "": nothing; "savgol": the Savitzky-Golay filter (window, polyorder) along the frames of all four columns;
    "savgol_center_and_constant_size": the same, then every frame gets the largest smoothed width and height times
    `over_crop_ratio`.  Then the reorder and the truncation toward zero.
    Deviation: the truncation makes a whole pixel of a difference in the last place -- a constant track of 40 comes back from
    the filter as 39.99999999999999 or 40.000000000000007 depending on how the coefficients were rounded -- so a smoothed value
    within 1e-6 below an integer counts as that integer.  ValueError for an unknown mode or fewer frames than the window."""
    if smoothing not in SMOOTHINGS:
        raise ValueError(f"smoothing must be one of {SMOOTHINGS}, got {smoothing!r}")
    b = np.array(boxes, dtype=np.float64)
    if b.ndim != 2 or b.shape[1] != 4 or b.shape[0] < 1:
        raise ValueError(f"boxes must have shape (F, 4), got {b.shape}")
    b[:, 0] += b[:, 2] // 2
    b[:, 1] += b[:, 3] // 2
    if smoothing:
        if b.shape[0] < int(window):
            raise ValueError(f"a clip of {b.shape[0]} frames is shorter than the window of {window}")
        b = _savgol_apply(b, int(window), int(polyorder))
        if smoothing == "savgol_center_and_constant_size":
            b[:, 2] = b[:, 2].max() * over_crop_ratio
            b[:, 3] = b[:, 3].max() * over_crop_ratio
        up = np.ceil(b)
        b = np.where(up - b < SNAP, up, b)
    return np.stack([b[:, 3], b[:, 2], b[:, 0], b[:, 1]], 1).astype(np.int32)


def crop_transforms(hwcxcy, out_size=256, margin=1.15):
    """(F, 4) boxes as h, w, cx, cy (`smooth_boxes`) -> float64 (F, 2, 3): the forward transform (frame -> crop) that `crop_v2`
    returns for `crop_img(smooth_filter=True)`: scale = max(w - 1, h - 1) / 200, get_affine_transform(center = (cx, cy),
    scale * margin, rot = 0, (S, S)).  That function rounds three source points to float32,
        P0 = (cx, cy),  P1 = (cx, y1), y1 = fl32(cy - 0.5 s),  P2 = (x2, y1), x2 = fl32(cx - fl32(cy - y1)),   s = 200 scale margin,
    sends them to (S/2, S/2), (S/2, 0), (0, 0) and solves for the six numbers.  P0, P1 share x and P1, P2 share y, so the
    solution is [[g, 0, -g x2], [0, k, -k y1]] with g = (S/2) / (cx - x2), k = (S/2) / (cy - y1); written as
    -(S/2 x2) / (cx - x2), whose numerator and denominator are exact in double, each entry is rounded once.
    out_size: 224 under the reference's SPECTRE flag, 256 otherwise; anything in [1, ops.CROP_MAX_SIDE].
    ValueError for a box whose larger side is below 2 (its three points coincide)."""
    b = np.asarray(hwcxcy)
    if b.ndim != 2 or b.shape[1] != 4:
        raise ValueError(f"boxes must have shape (F, 4) as h, w, cx, cy, got {b.shape}")
    S = int(out_size)
    if S != out_size or not 1 <= S <= ops.CROP_MAX_SIDE:
        raise ValueError(f"out_size must be an integer in [1, {ops.CROP_MAX_SIDE}], got {out_size!r}")
    b = b.astype(np.float64)
    side = np.maximum(b[:, 1] - 1.0, b[:, 0] - 1.0)
    if not (np.isfinite(b).all() and (side >= 1.0).all()):
        raise ValueError("crop_transforms: every box needs finite numbers and a side of at least 2 pixels")
    s = (side / 200.0 * margin) * 200.0                       # scale_tmp[0]
    cx, cy = b[:, 2].astype(np.float32), b[:, 3].astype(np.float32)
    y1 = (b[:, 3] + s * -0.5).astype(np.float32)
    x2 = cx - (cy - y1)                                       # float32 arithmetic, as get_3rd_point's
    assert x2.dtype == np.float32
    half = S * 0.5
    dx, dy = cx.astype(np.float64) - x2.astype(np.float64), cy.astype(np.float64) - y1.astype(np.float64)
    if not ((dx > 0).all() and (dy > 0).all()):
        raise ValueError("crop_transforms: a box is too small against its centre for float32 source points")
    trans = np.zeros((b.shape[0], 2, 3), np.float64)
    trans[:, 0, 0] = half / dx
    trans[:, 0, 2] = -(half * x2.astype(np.float64)) / dx
    trans[:, 1, 1] = half / dy
    trans[:, 1, 2] = -(half * y1.astype(np.float64)) / dy
    return trans


def _pair(points, trans):
    """(points, A (..., 2, 2), t (..., 2)) in one array library: torch if the points are a tensor, else numpy float64."""
    if torch.is_tensor(points):
        tr = trans.to(points) if torch.is_tensor(trans) else torch.as_tensor(np.asarray(trans), dtype=points.dtype, device=points.device)
    else:
        points = np.asarray(points, np.float64)
        tr = np.asarray(trans.detach().cpu() if torch.is_tensor(trans) else trans, dtype=np.float64)
    if tr.shape[-2:] != (2, 3) or points.shape[-1] != 2 or not (tr.ndim == 2 or (tr.ndim == 3 and points.ndim == 3
                                                                                 and tr.shape[0] == points.shape[0])):
        raise ValueError(f"points {tuple(points.shape)} and trans {tuple(tr.shape)}: want (P, 2) with (2, 3), or (F, P, 2) with "
                         "(2, 3) or (F, 2, 3)")
    return points, tr[..., :2], tr[..., 2]


def frame_to_crop(points, trans):
    """Frame pixels (F, P, 2) or (P, 2) as x, y -> crop pixels: points @ A^T + t per frame (the reference's
    transform_pixel_v2), with trans (F, 2, 3) or (2, 3) = [A | t].  numpy float64 in and out, or torch in the points' dtype."""
    p, A, t = _pair(points, trans)
    return (p[..., None, :] * A[..., None, :, :]).sum(-1) + t[..., None, :]


def crop_to_frame(points, trans):
    """The inverse of `frame_to_crop` (transform_pixel_v2(inverse=True)): (points - t) @ A^-T, A inverted by its 2 x 2 closed form."""
    p, A, t = _pair(points, trans)
    det = A[..., 0, 0] * A[..., 1, 1] - A[..., 0, 1] * A[..., 1, 0]
    q = p - t[..., None, :]
    x = (A[..., 1, 1, None] * q[..., 0] - A[..., 0, 1, None] * q[..., 1]) / det[..., None]
    y = (A[..., 0, 0, None] * q[..., 1] - A[..., 1, 0, None] * q[..., 0]) / det[..., None]
    return torch.stack([x, y], -1) if torch.is_tensor(p) else np.stack([x, y], -1)


def invert_transforms(trans):
    """float64 (F, 2, 3) forward transforms -> the inverse maps (crop -> frame) the kernel takes, by the 2 x 2 closed form in
    float64.  ValueError for a transform that is not finite or whose determinant is 0 (or so small that the inverse is not finite)."""
    tr = np.asarray(trans.detach().cpu() if torch.is_tensor(trans) else trans, dtype=np.float64)
    if tr.ndim != 3 or tr.shape[1:] != (2, 3):
        raise ValueError(f"trans must have shape (F, 2, 3), got {tr.shape}")
    a, b, c, d = tr[:, 0, 0], tr[:, 0, 1], tr[:, 1, 0], tr[:, 1, 1]
    det = a * d - b * c
    inv = np.empty_like(tr)
    with np.errstate(all="ignore"):
        inv[:, 0, 0], inv[:, 0, 1], inv[:, 1, 0], inv[:, 1, 1] = d / det, -b / det, -c / det, a / det
        inv[:, 0, 2] = -(inv[:, 0, 0] * tr[:, 0, 2] + inv[:, 0, 1] * tr[:, 1, 2])
        inv[:, 1, 2] = -(inv[:, 1, 0] * tr[:, 0, 2] + inv[:, 1, 1] * tr[:, 1, 2])
    if not np.isfinite(tr).all() or (det == 0).any() or not np.isfinite(inv).all():
        raise ValueError("crop_faces: a transform is not finite or is singular")
    return inv


def normalise_table(mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """(3, 256) fp32 on the host: row c holds (byte / 255 - mean[c]) / std[c] for every byte, in torch's own fp32 expression --
    ToTensor's `.float().div(255)` and Normalize's `.sub_(mean).div_(std)` -- so a lookup equals the reference's transform."""
    mean, std = torch.tensor(mean, dtype=torch.float32), torch.tensor(std, dtype=torch.float32)
    if mean.shape != (3,) or std.shape != (3,) or not (std != 0).all():
        raise ValueError("mean and std must hold three numbers each, std none of them 0")
    u8 = torch.arange(256, dtype=torch.uint8)
    return ((u8.float() / 255)[None, :] - mean[:, None]) / std[:, None]


def crop_faces(frames, trans, out_size=256, mean=IMAGENET_MEAN, std=IMAGENET_STD, dtype=torch.float32, swap_rb=True,
               return_uint8=False):
    """frames (F, H, W, 3 | 4) uint8 on the device (a row stride larger than the row and the renderer's RGBA view are taken as
    `ops.jpeg_encode` takes them; alpha is ignored), trans float64 (F, 2, 3) on the host (`crop_transforms`, or any affine
    map frame -> crop) -> (F, 3, S, S) in `dtype` (fp32, bf16 or fp16): the crop `cv2.warpAffine(frame, trans, (S, S),
    INTER_LINEAR)` describes (zero border; the operator of include/msmd_hip.h, not cv2's fixed-point one), channels swapped
    (`swap_rb`: the reference's cvtColor(RGB2BGR)), then (byte / 255 - mean[c]) / std[c] with c the channel after the swap.
    return_uint8: also the (F, S, S, 3) uint8 crop, channels in the same order.  ValueError for a transform that is not
    finite or singular."""
    inv = invert_transforms(trans)
    if not torch.is_tensor(frames) or not frames.is_cuda:
        raise TypeError("frames must be a uint8 tensor on the MI355X (cuda) device; there is no CPU path")
    if frames.dim() != 4 or inv.shape[0] != frames.shape[0]:
        raise ValueError(f"{inv.shape[0]} transforms for frames of shape {tuple(frames.shape)}")
    dev = frames.device
    out, crop = ops.face_crop(frames, torch.from_numpy(inv).to(dev), normalise_table(mean, std).to(dev), int(out_size), dtype=dtype,
                              swap_rb=swap_rb, want_uint8=return_uint8)
    return (out, crop) if return_uint8 else out


def clip_transforms(boxes, out_size=256, smoothing="savgol", K=5):
    """Detections or boxes of a clip -> float64 (F, 2, 3): `track_boxes` (if `boxes` is Step 1's list of detection lists and
    not an (F, 4) array of x, y, w, h), `smooth_boxes`, `crop_transforms`."""
    if not (isinstance(boxes, np.ndarray) or torch.is_tensor(boxes)):
        rows = list(boxes)
        detections = any(len(r) == 0 or isinstance(r[0], (tuple, list)) for r in rows)       # [] or [(face_id, box), ...]
        boxes = track_boxes(rows, K)[0] if detections else np.array([np.asarray(r, np.float64) for r in rows])
    boxes = np.asarray(boxes.detach().cpu() if torch.is_tensor(boxes) else boxes, dtype=np.float64)
    return crop_transforms(smooth_boxes(boxes, smoothing), out_size)


def crop_clip(frames, boxes, out_size=256, smoothing="savgol", batch_size=32, K=5, **crop_args):
    """Step 3's loop without the encoder: yields (batch (n, 3, S, S), trans (n, 2, 3)) over the frames of a clip, n =
    `batch_size` but for the last.  boxes: Step 1's `raw_bbox_frames` or an (F, 4) array of x, y, w, h (`processed_bbox_frames`);
    as in the reference, the shorter of frames and boxes ends the clip.  crop_args go to `crop_faces` (with return_uint8 the
    first item of a pair is itself a pair)."""
    trans = clip_transforms(boxes, out_size, smoothing, K)
    n = min(trans.shape[0], frames.shape[0])
    for i in range(0, n, int(batch_size)):
        j = min(i + int(batch_size), n)
        yield crop_faces(frames[i:j], trans[i:j], out_size, **crop_args), trans[i:j]


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="normalised face crops of a clip from its frames and Step 1's box pickle")
    p.add_argument("--frames", required=True, help=".npy, (F, H, W, 3) uint8, or a Motion-JPEG .avi (decoded on the device)")
    p.add_argument("--boxes", required=True, help="Step 1's .pickle: processed_bbox_frames if present, else raw_bbox_frames")
    p.add_argument("--out", required=True, help=".npy to write, (F, 3, S, S) float32")
    p.add_argument("--size", type=int, default=256, help="224 for the reference's SPECTRE flag")
    p.add_argument("--smoothing", default="savgol", choices=SMOOTHINGS)
    p.add_argument("--batch_size", type=int, default=32)
    p.add_argument("--video", default=None, help="also write the uint8 crops as a Motion-JPEG .avi")
    p.add_argument("--fps", type=float, default=None,
                   help="frame rate of --video (default: the pickle's fps, else the rate of an .avi given as --frames, else 30)")
    p.add_argument("--device", default="cuda")
    return p.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    file_fps = None
    if args.frames.lower().endswith(".avi"):
        from .media import read_avi, read_video
        frames, file_fps = read_video(args.frames, device=args.device), read_avi(args.frames).fps
    else:
        frames = torch.from_numpy(np.load(args.frames)).to(args.device)
    with open(args.boxes, "rb") as f:
        meta = pkl.load(f)
    boxes = meta["processed_bbox_frames"] if "processed_bbox_frames" in meta else meta["raw_bbox_frames"]
    outs, jpegs = [], []
    for item, _ in crop_clip(frames, boxes, args.size, args.smoothing, args.batch_size, return_uint8=args.video is not None):
        if args.video is not None:
            from .media import encode_jpeg
            item, crop = item
            jpegs += encode_jpeg(crop.flip(-1))       # back to the frames' channel order
        outs.append(item.cpu())
    out = torch.cat(outs).numpy()
    np.save(args.out, out)
    print(f"wrote {args.out}: {out.shape}")
    if args.video is not None:
        from .media import write_avi
        fps = args.fps if args.fps is not None else meta.get("fps", 30 if file_fps is None else file_fps)
        n = write_avi(args.video, jpegs, fps, (args.size, args.size))
        print(f"wrote {args.video}: {len(jpegs)} frames, {n} bytes")


if __name__ == "__main__":
    main()
