"""Records tests/golden/g13_headpose.npz: the REFERENCE head-pose stage (dataset_processing/Step2_preprocess_head_pose_mediapipe.py)
run on synthetic landmark clips.

    python tests/golden/make_goldens_headpose.py /path/to/reference/checkout

The script cannot be imported (cv2 / mediapipe): `procrustes_analysis`, `rotateToNeutral`, `smooth_rotation_matrices` and
`interpolate_landmarks` are built from its AST at recording time only and run with the installed scipy (1.15.3 at recording; the archive notes it); the dozen lines of its
`__main__` tail (R_adjust, as_euler('YXZ'), roll = -roll, R_modified) are restated here with scipy.  The archive holds data
only: the canonical face's vertices and the static indices (the reference's assets), inputs that are exactly representable in
fp32, the reference's outputs, scipy's Savitzky-Golay coefficients and filter outputs, and the error of the same functions on
float32 copies of the inputs.  tests/test_headpose_cpu.py pins tests/headpose_ref.py's restatement to these values."""
import ast
import json
import os
import sys

import numpy as np
import scipy
from scipy.signal import savgol_coeffs, savgol_filter
from scipy.spatial.transform import Rotation

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import headpose_ref as HR  # noqa: E402

STEP2 = "dataset_processing/Step2_preprocess_head_pose_mediapipe.py"
GEOM = "dataset_processing/models/mediapipe_geometries"
NAMES = ("procrustes_analysis", "rotateToNeutral", "smooth_rotation_matrices", "interpolate_landmarks")
PAIRS = ((5, 2), (7, 3), (9, 4))


def load_reference(ref_root):
    tree = ast.parse(open(os.path.join(ref_root, STEP2)).read())
    keep = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in NAMES]
    ns = dict(np=np, Rotation=Rotation, savgol_filter=savgol_filter)
    exec(compile(ast.Module(body=keep, type_ignores=[]), "<reference Step2>", "exec"), ns)
    return [ns[n] for n in NAMES]


def load_assets(ref_root):
    verts = [list(map(float, ln.split()[1:4])) for ln in open(os.path.join(ref_root, GEOM, "mediapipe_canonical_face_mesh.obj"),
                                                              errors="replace") if ln.startswith("v ")]
    m = json.load(open(os.path.join(ref_root, GEOM, "mediapipe_emantic_mapping.json")))
    return np.array(verts, np.float32), np.array(m["nose"]["dorsum"] + m["nose"]["tipLower"] + m["additional_anchors"], np.int32)


def clip(rng, neutral, yaw, pitch, roll, mirror=False, noise=2e-4):
    """Landmarks (F, N, 3) fp32: the neutral points under poses chosen so that the final angles come out near (yaw, pitch,
    -roll): x = s Rp n + (0.5, 0.5, 0) + noise with Rp = Rpose^T Rx(180)."""
    F = len(yaw)
    Rpose = Rotation.from_euler("YXZ", np.stack([yaw, pitch, roll], 1), degrees=True).as_matrix()
    Rx = np.diag([1.0, -1.0, -1.0])
    L = np.zeros((F, neutral.shape[0], 3))
    for f in range(F):
        L[f] = (neutral.astype(np.float64) @ (Rpose[f].T @ Rx).T) / 30.0 + np.array([0.5, 0.5, 0.0])
    L += noise * rng.standard_normal(L.shape)
    if mirror:
        L[..., 0] = 1.0 - L[..., 0]
    return L.astype(np.float32)


def run_reference(fns, L32, valid, neutral, static_idx, dtype):
    procrustes_analysis, rotateToNeutral, smooth_rotation_matrices, interpolate_landmarks = fns
    frames = [L32[f].astype(dtype) if valid[f] else None for f in range(len(valid))]
    filled, _ = interpolate_landmarks(frames)
    filled = np.array(filled)
    aligned, R, t = rotateToNeutral(neutral.astype(dtype), filled, list(static_idx), returnRotation=True)
    c = np.array([procrustes_analysis(filled[f, static_idx].T, neutral.astype(dtype)[static_idx].T)[1] for f in range(len(valid))])
    R_smooth = np.array(smooth_rotation_matrices(R, window_length=5, polyorder=2))
    # the __main__ tail, restated
    R_adjust = Rotation.from_euler('X', 180, degrees=True).as_matrix()
    ypr, R_mod = [], []
    for Rc in R_smooth:
        yaw, pitch, roll = Rotation.from_matrix(R_adjust @ Rc).as_euler('YXZ', degrees=True)
        roll = -roll
        ypr.append([yaw, pitch, roll])
        R_mod.append(Rotation.from_euler('YXZ', [yaw, pitch, roll], degrees=True).as_matrix())
    return dict(filled=filled, R=np.array(R), c=c, t=np.array(t)[:, :, 0], aligned=np.asarray(aligned), R_smooth=R_smooth,
                ypr=np.array(ypr), R_modified=np.array(R_mod))


def savgol_longdouble(x, w, p):
    """The filter's definition in long double: Gram-Schmidt (twice) on the Vandermonde matrix, H = Q Q^T."""
    h, F = w // 2, x.shape[0]
    A = (np.arange(w, dtype=np.longdouble) - h)[:, None] ** np.arange(p + 1)[None, :]
    Q = np.zeros_like(A)
    for k in range(p + 1):
        v = A[:, k].copy()
        for _ in range(2):
            for j in range(k):
                v -= (Q[:, j] @ v) * Q[:, j]
        Q[:, k] = v / np.sqrt(v @ v)
    H = Q @ Q.T
    y = np.zeros(x.shape, np.longdouble)
    for j in range(F):
        y[j] = H[j] @ x[:w] if j < h else H[w - h + j - (F - h)] @ x[F - w:] if j >= F - h else H[h] @ x[j - h:j + h + 1]
    return y


def main(ref_root):
    fns = load_reference(ref_root)
    canon, static = load_assets(ref_root)
    assert canon.shape == (468, 3) and static.shape == (20,)
    rng = np.random.default_rng(20240613)
    out = {"canonical": canon, "static_idx": static}
    # 478 tracked points: the 468 vertices and ten more (iris), here copies of ten vertices pushed along z
    extra = canon[[468 - 10 + k for k in range(10)]] + np.float32([0, 0, 0.5])
    neutral478 = np.concatenate([canon, extra], 0)
    small = np.concatenate([static, np.arange(200, 210, dtype=np.int32)])           # P = 30: the static points first
    u = lambda F: np.linspace(0, 1, F)
    cases = {}
    # 37 frames, 8 missing: 1 at the start, gaps of 1 / 2 / 3 inside, 1 at the end
    F = 37
    valid = np.ones(F, bool)
    valid[[0, 5, 10, 11, 20, 21, 22, 36]] = False
    cases["clip37"] = (clip(rng, neutral478, 35 * np.sin(2 * np.pi * u(F)), 20 * np.cos(3 * u(F)), 15 * np.sin(5 * u(F))),
                       valid, neutral478, static)
    F = 12
    cases["mirror"] = (clip(rng, canon[small], 20 * u(F) - 10, 10 * np.sin(4 * u(F)), 8 * u(F), mirror=True),
                       np.ones(F, bool), canon[small], np.arange(20, dtype=np.int32))
    F = 24
    cases["flip"] = (clip(rng, canon[small], 250 * u(F) - 125, 30 * np.sin(6 * u(F)), 20 * np.cos(4 * u(F))),
                     np.ones(F, bool), canon[small], np.arange(20, dtype=np.int32))
    need_flip, neg_det = False, False
    for name, (L32, valid, neutral, sidx) in cases.items():
        r64 = run_reference(fns, L32, valid, neutral, sidx, np.float64)
        r32 = run_reference(fns, L32, valid, neutral, sidx, np.float32)
        assert np.abs(r64["ypr"][:, 1]).max() <= 60.0, name
        for f in range(len(valid)):
            X, Y = r64["filled"][f, sidx], neutral.astype(np.float64)[sidx]
            cov = (Y - Y.mean(0)).T @ (X - X.mean(0)) / len(sidx)
            sv = np.linalg.svd(cov, compute_uv=False)
            assert sv[2] > 0.05 * sv[0], (name, f, sv)
            neg_det |= bool(np.linalg.det(cov) < 0)
        q = np.array([Rotation.from_matrix(m).as_quat() for m in r64["R"]])
        need_flip |= bool(((q[1:] * q[:-1]).sum(1) < 0).any())
        # numpy's linspace(...).astype(int) must land on start+1 .. end-1 for every gap used
        idx = np.flatnonzero(valid)
        for a, b in zip(idx[:-1], idx[1:]):
            if b - a > 1:
                assert np.array_equal(np.linspace(a + 1, b - 1, b - a - 1).astype(int), np.arange(a + 1, b)), (name, a, b)
        rel = lambda x, y: float(np.abs(x.astype(np.float64) - y).max() / np.abs(y).max())
        err32 = np.array([HR.geodesic_deg(r32["R"], r64["R"]).max(), rel(r32["c"], r64["c"]), rel(r32["t"], r64["t"]),
                          rel(r32["aligned"], r64["aligned"])])
        print(f"{name}: F = {len(valid)}, err32_fit (R deg, c rel, t rel, aligned rel) = {err32}, "
              f"float32 angles err = {np.abs(r32['ypr'] - r64['ypr']).max():.2e} deg")
        out[f"{name}/landmarks"] = L32
        out[f"{name}/valid"] = valid
        out[f"{name}/neutral"] = neutral
        out[f"{name}/static_idx"] = sidx
        miss = np.flatnonzero(~valid)
        out[f"{name}/filled_missing"] = r64["filled"][miss]
        keep = np.unique(np.concatenate([miss[:2], [0, len(valid) // 2, len(valid) - 1]])) if L32.shape[1] > 100 else np.arange(len(valid))
        out[f"{name}/aligned_frames"] = keep
        out[f"{name}/aligned"] = r64["aligned"][keep]
        for k in ("R", "c", "t", "R_smooth", "ypr", "R_modified"):
            out[f"{name}/{k}"] = r64[k]
        out[f"{name}/err32_fit"] = err32
    assert need_flip, "no case needs a quaternion sign flip"
    assert neg_det, "no case has det(cov) < 0"
    out["cases"] = np.array(list(cases))
    # Samples in [-1, 1): an absolute bound on the filter's output is then a relative one too.  scipy fits its edge polynomials
    # with np.polyfit on the positions 0 .. w-1, which costs it digits at (9, 4); its own distance from a long-double evaluation
    # of the definition is asserted to stay below half of the 1e-13 the test allows, so that the test measures the table.
    x = rng.uniform(-1.0, 1.0, (12, 4))
    out["savgol/x"] = x
    for w, p in PAIRS:
        out[f"savgol/coeffs_{w}_{p}"] = savgol_coeffs(w, p)
        out[f"savgol/y_{w}_{p}"] = y = savgol_filter(x, w, p, axis=0, mode="interp")
        own = float(np.abs(y - savgol_longdouble(x, w, p)).max())
        print(f"savgol ({w}, {p}): scipy against the long-double definition {own:.2e}")
        assert own <= 0.5e-13, own
    assert np.allclose(out["savgol/coeffs_5_2"] * 35, [-3, 12, 17, 12, -3], rtol=0, atol=1e-13)
    out["versions"] = np.array(json.dumps({"numpy": np.__version__, "scipy": scipy.__version__, "python": sys.version.split()[0]}))
    path = os.path.join(HERE, "g13_headpose.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(out)} arrays, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main(sys.argv[1])
