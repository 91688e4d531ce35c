"""Records tests/golden/g16_face_crop.npz: the REFERENCE's box tracker (dataset_processing/Step1_preprocess_boundbox_mediapipe.py:
filter_boxes), its crop arithmetic (Step3_preprocess_expression_code.py: crop_img; transform.py: get_affine_transform) and
scipy's box smoothing, run on synthetic detections and boxes.

    python tests/golden/make_goldens_face_crop.py /path/to/reference/checkout

The scripts cannot be imported (cv2 / mediapipe / torchvision): the functions are built from their AST at recording time only.
`cv2.getAffineTransform` does not exist here and is stubbed twice: by an exact rational solve of the float32 points
(fractions.Fraction) rounded once to double -- the truth -- and by np.linalg.solve, whose deviation from the truth (err_lu) is
the yardstick for the product's closed form.  Step 3's box smoothing lives in its `__main__` (lines 196-218) and is restated
here with scipy.  The archive holds data only: detections, boxes, the functions' outputs and notes."""
import ast
import json
import math
import os
import sys
from fractions import Fraction
from types import SimpleNamespace

import numpy as np
import scipy
from scipy.interpolate import interp1d
from scipy.signal import savgol_filter

HERE = os.path.dirname(os.path.abspath(__file__))
STEP1 = "dataset_processing/Step1_preprocess_boundbox_mediapipe.py"
STEP3 = "dataset_processing/Step3_preprocess_expression_code.py"
TRANSFORM = "dataset_processing/transform.py"
MODES = ("", "savgol", "savgol_center_and_constant_size")


def functions(ref_root, rel, names, ns):
    tree = ast.parse(open(os.path.join(ref_root, rel)).read())
    keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    keep = [n for i, n in enumerate(keep) if n.name not in [m.name for m in keep[:i]]]        # Step 1 defines calculate_iou twice
    exec(compile(ast.Module(body=keep, type_ignores=[]), f"<reference {rel}>", "exec"), ns)
    return ns


def solve_exact(src, dst):
    """The 2 x 3 map that takes the three float32 points src to dst, solved over the rationals and rounded once."""
    P = [[Fraction(float(v)) for v in row] + [Fraction(1)] for row in src]
    det = lambda m: (m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0])
                     + m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]))
    D = det(P)
    out = np.zeros((2, 3))
    for r in range(2):
        u = [Fraction(float(dst[i][r])) for i in range(3)]
        for k in range(3):
            m = [row[:] for row in P]
            for i in range(3):
                m[i][k] = u[i]
            out[r, k] = float(det(m) / D)
    return out


def solve_lu(src, dst):
    A = np.concatenate([np.asarray(src, np.float64), np.ones((3, 1))], 1)
    return np.linalg.solve(A, np.asarray(dst, np.float64)).T


def detections(frames):
    """A list per frame of (face_id, (x, y, w, h)) -> int64 (n, 6) rows of frame, face_id, x, y, w, h."""
    return np.array([[f, fid, *box] for f, dets in enumerate(frames) for fid, box in dets], np.int64).reshape(-1, 6)


def tracker_cases():
    def walk(F, x=600, y=200, w=300, h=320, dx=3, dy=-2):
        return [[(0, (x + dx * f + (f * f) % 5, y + dy * f + (3 * f) % 4, w + f % 3, h - f % 2))] for f in range(F)]
    other = lambda f: (1, (1300 - 2 * f, 400 + f, 200, 210))
    cases = {"one_face": walk(8)}
    c = walk(9); c[4] = []; cases["gap1"] = c
    c = walk(7); c[0] = []; cases["first_missing"] = c
    c = walk(7); c[-1] = []; cases["last_missing"] = c
    c = walk(10); c[7] = [other(7), c[7][0]]; cases["two_faces_mid_above"] = c           # the true face is listed second
    c = walk(10, dx=70); c[7] = [c[7][0], other(7)]; cases["two_faces_mid_below"] = c    # fast motion: mean IoU below 0.4
    c = walk(6, dx=0, dy=0); c[2] = [c[2][0], other(2)]; cases["two_faces_early"] = c     # two frames before it: divided by K all the same
    for ahead in (0, 1, 3):
        c = walk(9)
        for f in range(9):
            if f == 0 or f > ahead:
                c[f] = [other(f), c[f][0]]
        cases[f"first_two_ahead{ahead}"] = c
    return cases


def clear_column(rng, F, start, step, extra=()):
    """An integer track whose (5, 2)-filtered values all stay 1e-3 away from every integer (the filter's coefficients are
    multiples of 1 / 35 and 1 / 70, so a random integer track lands on integers now and then): drawn until that holds."""
    while True:
        col = start + np.cumsum(rng.integers(-step, step + 1, F))
        y = savgol_filter(col.astype(np.float64), 5, 2)
        vals = np.concatenate([y] + [np.atleast_1d(f(y)) for f in extra])
        if np.abs(vals - np.rint(vals)).min() > 1e-3:
            return col


def main(ref_root):
    out = {}
    # ---- Step 1: the tracker
    s1 = functions(ref_root, STEP1, ("calculate_iou", "filter_boxes"), dict(np=np, interp1d=interp1d))
    cases = tracker_cases()
    for name, frames in cases.items():
        boxes, flag = s1["filter_boxes"]([list(f) for f in frames], 5)
        boxes = np.array([np.asarray(b, np.float64) for b in boxes])
        assert boxes.shape == (len(frames), 4), (name, boxes.shape)
        out[f"track/{name}/n_frames"] = np.array(len(frames))
        out[f"track/{name}/detections"] = detections(frames)
        out[f"track/{name}/boxes"] = boxes
        out[f"track/{name}/flags"] = np.array(json.dumps(flag))
        print(name, flag)
    assert json.loads(str(out["track/two_faces_mid_above/flags"]))["has_multiple"]
    assert np.array_equal(out["track/two_faces_mid_above/boxes"][7], cases["two_faces_mid_above"][7][1][1])
    assert np.array_equal(out["track/two_faces_mid_below/boxes"][7], out["track/two_faces_mid_below/boxes"][6])
    assert np.array_equal(out["track/two_faces_early/boxes"][2], out["track/two_faces_early/boxes"][1])
    out["track/cases"] = np.array(list(cases))
    c = cases["gap1"][:]
    c[5] = []
    try:
        s1["filter_boxes"]([list(f) for f in c], 5)
        note = "no exception"
    except Exception as e:                                        # noqa: BLE001
        note = f"{type(e).__name__}: {e}"
    print("two-frame gap under numpy", np.__version__, "->", note)
    out["track/gap2_note"] = np.array(note)
    # ---- Step 3, lines 196-218: box smoothing (restated with scipy)
    rng = np.random.default_rng(20240716)
    lengths = (5, 6, 40)
    for F in lengths:
        # columns x, y, w, h; cx = x + w // 2 is what the filter sees, so the clear columns are drawn for cx, cy, w, h
        w = clear_column(rng, F, 300, 4, extra=(lambda y: y.max() * 1.2,))
        h = clear_column(rng, F, 330, 4, extra=(lambda y: y.max() * 1.2,))
        cx, cy = clear_column(rng, F, 900, 6), clear_column(rng, F, 420, 5)
        boxes = np.stack([cx - w // 2, cy - h // 2, w, h], 1).astype(np.int64)
        out[f"smooth/{F}/boxes"] = boxes
        for m, mode in enumerate(MODES):
            bb = np.array(boxes)
            bb[:, 0] = bb[:, 0] + bb[:, 2] // 2
            bb[:, 1] = bb[:, 1] + bb[:, 3] // 2
            if mode == "":
                sm = bb
            else:
                sm = savgol_filter(bb, 5, 2, axis=0)
                if mode == "savgol_center_and_constant_size":
                    sm[:, 2], sm[:, 3] = np.max(sm[:, 2]) * 1.2, np.max(sm[:, 3]) * 1.2
                assert np.abs(sm - np.rint(sm)).min() > 1e-6, (F, mode)          # the parity inputs stay clear of the snap rule
            sm = np.array([sm[:, 3], sm[:, 2], sm[:, 0], sm[:, 1]]).T
            if m == 1:
                out[f"smooth/{F}/savgol_float"] = sm.astype(np.float64)
            out[f"smooth/{F}/mode{m}"] = sm.astype(np.int32)
    out["smooth/lengths"] = np.array(lengths)
    const = np.tile(np.array([[40.0, 41.0, 300.0, 7.0]]), (9, 1))
    out["smooth/constant_in"] = const
    out["smooth/constant_scipy"] = savgol_filter(const, 5, 2, axis=0)
    print("scipy on a constant track:", [repr(float(v)) for v in np.unique(out["smooth/constant_scipy"])])
    # ---- Step 3: crop_img's box arithmetic; transform.py: get_affine_transform
    calls = []
    cv2 = SimpleNamespace(getAffineTransform=None, warpAffine=lambda img, trans, size, flags=None: None, INTER_LINEAR=1,
                          cvtColor=lambda img, code: img, COLOR_RGB2BGR=4)
    tf = functions(ref_root, TRANSFORM, ("get_3rd_point", "get_affine_transform", "get_dir", "crop_v2"), dict(np=np, cv2=cv2))

    def crop_v2(img, center, scale, size):
        calls.append((np.array(center), float(scale), tuple(size)))
        return tf["crop_v2"](img, center, scale, size)
    args = SimpleNamespace(get_processed_videos_spectre=False)
    s3 = functions(ref_root, STEP3, ("crop_img",), dict(np=np, cv2=cv2, math=math, crop_v2=crop_v2, args=args))
    tensor = lambda img: SimpleNamespace(unsqueeze=lambda dim: None)
    boxes = np.array([(2, 2, 960, 540), (3, 3, 5, 7), (200, 200, 960, 540), (1079, 1079, 960, 540), (150, 200, 100, 1000),
                      (200, 150, 1900, 20), (300, 2, -40, 500), (3, 640, 2000, -15), (1079, 607, 959, 541), (431, 433, 1, 1079),
                      (2, 3, 1919, 1079), (640, 1079, 2500, 1300)], np.int32)                    # h, w, cx, cy
    sizes = (224, 256)
    truth, lu = np.zeros((2, len(boxes), 2, 3)), np.zeros((2, len(boxes), 2, 3))
    for si, S in enumerate(sizes):
        args.get_processed_videos_spectre = S == 224
        for solver, dest in ((solve_exact, truth), (solve_lu, lu)):
            cv2.getAffineTransform = solver
            for k, b in enumerate(boxes):
                calls.clear()
                dest[si, k] = s3["crop_img"](None, b, tensor)[1]
                assert calls[0][2] == (S, S)
                if si == 0 and solver is solve_exact:
                    out.setdefault("tf/center", np.zeros((len(boxes), 2)))[k] = calls[0][0]
                    out.setdefault("tf/scale", np.zeros(len(boxes)))[k] = calls[0][1]
    err = np.abs(lu - truth).max(-1) / np.abs(truth).max(-1)                                    # per row of each transform
    print(f"np.linalg.solve against the exact solve: err_lu max {err.max():.3e}, median {np.median(err):.3e}")
    out.update({"tf/boxes": boxes, "tf/sizes": np.array(sizes), "tf/truth": truth, "tf/lu": lu, "tf/err_lu": err})
    out["versions"] = np.array(json.dumps({"numpy": np.__version__, "scipy": scipy.__version__, "python": sys.version.split()[0]}))
    path = os.path.join(HERE, "g16_face_crop.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main(sys.argv[1])
