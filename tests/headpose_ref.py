"""Head pose from tracked face landmarks, restated in numpy from the definitions (no scipy): gap filling, the per-frame
similarity fit (Umeyama / Procrustes), quaternion sign continuity, the Savitzky-Golay filter with polynomial edge rows, the
180 degree turn about X and the intrinsic Y-X-Z angles.  Every function takes `dtype`, so the whole chain also runs in
float32: that run against the float64 one is the yardstick the GPU tests scale their bounds from.
tests/test_headpose_cpu.py pins the float64 run to the reference's recorded outputs (tests/golden/g13_headpose.npz)."""
import numpy as np


# ----------------------------------------------------------------------------------------------- gap filling
def gap_fill(landmarks, valid, dtype=np.float64):
    """Frames before the first / after the last valid frame copy it; missing frame i (from 0) of a gap of g between valid
    frames a < b is (1 - tau) L[a] + tau L[b] with tau = (i + 1) / (g + 2)."""
    L = np.array(landmarks, dtype=dtype)
    idx = np.flatnonzero(np.asarray(valid, bool))
    L[:idx[0]] = L[idx[0]]
    L[idx[-1] + 1:] = L[idx[-1]]
    for a, b in zip(idx[:-1], idx[1:]):
        g = b - a - 1
        for i in range(g):
            tau = (i + 1) / (g + 2)
            L[a + 1 + i] = dtype(1 - tau) * L[a] + dtype(tau) * L[b]
    return L


# ----------------------------------------------------------------------------------------------- the fit
def procrustes(X, Y, dtype=np.float64):
    """X, Y (S, 3): the similarity transform Y ~ c R X + t minimising the squared error (Umeyama 1991).  The sign matrix
    follows det(U) det(V^T); equal to the sign of det(cov) for a covariance of full rank."""
    X = np.asarray(X, dtype)
    Y = np.asarray(Y, dtype)
    S = X.shape[0]
    mu_x, mu_y = X.mean(0), Y.mean(0)
    xc, yc = X - mu_x, Y - mu_y
    rho2 = (xc * xc).sum(0) / dtype(S)
    rho2 = rho2.sum()
    cov = (yc.T @ xc) / dtype(S)
    U, D, Vt = np.linalg.svd(cov)
    s = np.ones(3, dtype)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        s[2] = -1
    R = (U * s) @ Vt
    c = (D * s).sum() / rho2
    t = mu_y - (c * R) @ mu_x
    return R.astype(dtype), dtype(c), t.astype(dtype)


def fit(landmarks, neutral, static_idx, dtype=np.float64):
    """landmarks (F, P, 3), neutral (N, 3) -> R (F, 3, 3), c (F), t (F, 3), aligned (F, P, 3) = c R x + t."""
    L = np.asarray(landmarks, dtype)
    Y = np.asarray(neutral, dtype)[static_idx]
    F = L.shape[0]
    R = np.zeros((F, 3, 3), dtype)
    c = np.zeros(F, dtype)
    t = np.zeros((F, 3), dtype)
    for f in range(F):
        R[f], c[f], t[f] = procrustes(L[f, static_idx], Y, dtype)
    aligned = np.einsum("fij,fpj->fpi", c[:, None, None] * R, L) + t[:, None, :]
    return R, c, t, aligned.astype(dtype)


# ----------------------------------------------------------------------------------------------- rotations
def mat_to_quat(R):
    """(F, 3, 3) -> (F, 4) in (x, y, z, w) order, unit norm; the branch with the largest of (m00, m11, m22, trace), which
    makes that component positive."""
    R = np.asarray(R)
    q = np.zeros((R.shape[0], 4), R.dtype)
    for f, m in enumerate(R):
        d = np.array([m[0, 0], m[1, 1], m[2, 2], m[0, 0] + m[1, 1] + m[2, 2]])
        k = int(np.argmax(d))
        if k == 3:
            q[f] = [m[2, 1] - m[1, 2], m[0, 2] - m[2, 0], m[1, 0] - m[0, 1], 1 + d[3]]
        else:
            i, j, l = k, (k + 1) % 3, (k + 2) % 3
            q[f, i] = 1 - d[3] + 2 * m[i, i]
            q[f, j] = m[j, i] + m[i, j]
            q[f, l] = m[l, i] + m[i, l]
            q[f, 3] = m[l, j] - m[j, l]
        q[f] /= np.sqrt((q[f] * q[f]).sum())
    return q


def continuous_signs(q):
    q = q.copy()
    for i in range(1, len(q)):
        if (q[i] * q[i - 1]).sum() < 0:
            q[i] = -q[i]
    return q


def quat_to_mat(q):
    x, y, z, w = (q[:, k] for k in range(4))
    R = np.empty((q.shape[0], 3, 3), q.dtype)
    R[:, 0, 0] = 1 - 2 * (y * y + z * z); R[:, 0, 1] = 2 * (x * y - z * w); R[:, 0, 2] = 2 * (x * z + y * w)
    R[:, 1, 0] = 2 * (x * y + z * w); R[:, 1, 1] = 1 - 2 * (x * x + z * z); R[:, 1, 2] = 2 * (y * z - x * w)
    R[:, 2, 0] = 2 * (x * z - y * w); R[:, 2, 1] = 2 * (y * z + x * w); R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def euler_yxz_deg(R):
    """Intrinsic Y-X-Z angles of R = Ry(yaw) Rx(pitch) Rz(roll), degrees: (F, 3) = yaw, pitch, roll."""
    pitch = np.arcsin(np.clip(-R[:, 1, 2], -1, 1))
    yaw = np.arctan2(R[:, 0, 2], R[:, 2, 2])
    roll = np.arctan2(R[:, 1, 0], R[:, 1, 1])
    return np.degrees(np.stack([yaw, pitch, roll], 1)).astype(R.dtype)


def euler_yxz_to_mat(deg):
    a = np.radians(deg)
    cy, sy, cx, sx, cz, sz = np.cos(a[:, 0]), np.sin(a[:, 0]), np.cos(a[:, 1]), np.sin(a[:, 1]), np.cos(a[:, 2]), np.sin(a[:, 2])
    R = np.empty((a.shape[0], 3, 3), a.dtype)
    R[:, 0, 0] = cy * cz + sy * sx * sz; R[:, 0, 1] = -cy * sz + sy * sx * cz; R[:, 0, 2] = sy * cx
    R[:, 1, 0] = cx * sz; R[:, 1, 1] = cx * cz; R[:, 1, 2] = -sx
    R[:, 2, 0] = -sy * cz + cy * sx * sz; R[:, 2, 1] = sy * sz + cy * sx * cz; R[:, 2, 2] = cy * cx
    return R


def geodesic_deg(Ra, Rb):
    """Angle of Ra^T Rb in degrees from the chord: |Ra - Rb|_F = 2 sqrt(2) sin(angle / 2) (no arccos near 1)."""
    d = np.asarray(Ra, np.float64) - np.asarray(Rb, np.float64)
    chord = np.sqrt((d * d).sum((-2, -1)))
    return np.degrees(2 * np.arcsin(np.minimum(chord / (2 * np.sqrt(2.0)), 1.0)))


# ----------------------------------------------------------------------------------------------- Savitzky-Golay
def savgol_table(window, polyorder):
    """-> (coeffs (w), edges (2 (w // 2), w)) float64 from the definition: with A the Vandermonde matrix of the w window
    positions (centred and scaled to [-1, 1]) and A = Q R, H = Q Q^T maps w samples to their least-squares polynomial
    evaluated at each position.  The centre row is the interior filter; rows 0 .. h-1 and w-h .. w-1 serve the first / last h
    frames (the polynomial fitted to the first / last w samples, evaluated at that frame)."""
    w, h = int(window), int(window) // 2
    pos = (np.arange(w, dtype=np.float64) - h) / h
    A = pos[:, None] ** np.arange(polyorder + 1)[None, :]
    Q = np.linalg.qr(A)[0]
    H = Q @ Q.T
    return H[h].copy(), np.concatenate([H[:h], H[w - h:]], 0)


def savgol_apply(x, window, polyorder, dtype=np.float64):
    """x (F, C), F >= window: the filter along axis 0."""
    coeffs, edges = savgol_table(window, polyorder)
    coeffs, edges = coeffs.astype(dtype), edges.astype(dtype)
    x = np.asarray(x, dtype)
    F, w, h = x.shape[0], window, window // 2
    y = np.zeros_like(x)
    for j in range(F):
        if j < h:
            y[j] = edges[j] @ x[:w]
        elif j >= F - h:
            y[j] = edges[h + j - (F - h)] @ x[F - w:]
        else:
            y[j] = coeffs @ x[j - h:j + h + 1]
    return y


def smooth(R, window=5, polyorder=2, dtype=np.float64):
    """R (F, 3, 3) raw fits -> dict: q (sign-continuous quaternions), R_smooth, ypr (F, 3) yaw / pitch / -roll in degrees,
    R_modified (rebuilt from ypr)."""
    R = np.asarray(R, dtype)
    q = continuous_signs(mat_to_quat(R))
    s = savgol_apply(q, window, polyorder, dtype)
    s = s / np.sqrt((s * s).sum(1, keepdims=True))
    R_smooth = quat_to_mat(s)
    adj = R_smooth * np.array([1, -1, -1], dtype)[None, :, None]
    ypr = euler_yxz_deg(adj)
    ypr[:, 2] = -ypr[:, 2]
    return dict(q=q, R_smooth=R_smooth, ypr=ypr, R_modified=euler_yxz_to_mat(ypr))


def head_pose(landmarks, neutral, static_idx, valid=None, window=5, polyorder=2, dtype=np.float64):
    """The whole chain for one clip -> dict(filled, R, c, t, aligned, ypr, R_smooth, R_modified)."""
    L = np.asarray(landmarks, dtype)
    if valid is not None:
        L = gap_fill(L, valid, dtype)
    R, c, t, aligned = fit(L, neutral, np.asarray(static_idx), dtype)
    out = smooth(R, window, polyorder, dtype)
    out.update(filled=L, R=R, c=c, t=t, aligned=aligned)
    return out
