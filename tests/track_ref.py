"""Float64 numpy restatement of the track resampler (csrc/track_resample.hip): scipy.signal.resample on a real
track as a dense two-stage DFT -- not np.fft -- with the twiddle phases reduced in integers, and the operator matrix W (M, F)
the error bound of tests/test_assemble_gpu.py is taken from.  The Savitzky-Golay matrix (scipy's mode='interp') composes in."""
import numpy as np


def twiddles(rows, cols, P):
    """e^{2 pi i (row * col mod P) / P} as (cos, sin), the residue exact in integers."""
    r = (np.asarray(rows, np.int64)[:, None] * np.asarray(cols, np.int64)[None, :]) % P
    ang = 2.0 * np.pi * r.astype(np.float64) / P
    return np.cos(ang), np.sin(ang)


def savgol_matrix(F, window, polyorder):
    """S (F, F): S @ x = savgol_filter(x, window, polyorder, axis=0, mode='interp').  Interior rows hold the centred least-squares
    polynomial's value at the window's middle, the first / last window // 2 rows the polynomial fitted to the first / last
    `window` samples evaluated at that frame."""
    if window % 2 == 0 or window < 3 or polyorder >= window or F < window:
        raise ValueError((F, window, polyorder))
    h = window // 2
    pos = (np.arange(window, dtype=np.float64) - h) / h
    A = pos[:, None] ** np.arange(polyorder + 1)[None, :]
    H = A @ np.linalg.pinv(A)                      # samples -> fitted polynomial at every position of the window
    S = np.zeros((F, F))
    for j in range(F):
        if j < h:
            S[j, :window] = H[j]
        elif j >= F - h:
            S[j, F - window:] = H[window - (F - j)]
        else:
            S[j, j - h:j + h + 1] = H[h]
    return S


def _stages(F, M):
    """(A_re, A_im) (K + 1, F) with X = (A_re + i A_im) x, and (S_re, S_im) (M, K + 1) with y = S_re X_re + S_im X_im: the
    Nyquist rule, the weights 1, 2, .., 2 and 1 / Nx sit in the synthesis stage."""
    Nx, num = int(F), int(M)
    N = min(Nx, num)
    K = N // 2
    k = np.arange(K + 1)
    ca, sa = twiddles(k, np.arange(Nx), Nx)        # e^{-i}: X = (ca - i sa) x
    cs, ss = twiddles(np.arange(num), k, num)      # e^{+i}: Re(X e) = X_re cs - X_im ss
    w = np.full(K + 1, 2.0)
    w[0] = 1.0
    if N % 2 == 0:
        w[K] *= 2.0 if num < Nx else (0.5 if num > Nx else 1.0)
    w_im = w.copy()
    if K > 0 and num % 2 == 0 and K == num // 2:   # the output's own Nyquist bin: once, real part only
        w[K] *= 0.5
        w_im[K] = 0.0
    return (ca, -sa), (cs * w / Nx, -ss * w_im / Nx)


def resample_matrix(F, M, smooth=None):
    """W (M, F) float64 with y = W @ x.  Nx = F, num = M, N = min(Nx, num), K = N // 2:
    X[k] = sum_n x[n] e^{-2 pi i k n / Nx}; N even: X[K] times 2 (num < Nx) or 0.5 (num > Nx);
    y[m] = (1 / Nx) Re(X[0] + 2 sum_{k=1..K} X[k] e^{+2 pi i k m / num}), bin K once and real when num is even and K == num / 2."""
    (a_re, a_im), (s_re, s_im) = _stages(F, M)
    W = s_re @ a_re + s_im @ a_im
    if smooth is not None:
        W = W @ savgol_matrix(int(F), *smooth)
    return W


def resample(x, M, smooth=None):
    """x (F, C) -> ((M, C) float64, W): the filter, the analysis and the synthesis applied one after the other."""
    x = np.asarray(x, np.float64)
    F = x.shape[0]
    xs = x if smooth is None else savgol_matrix(F, *smooth) @ x
    (a_re, a_im), (s_re, s_im) = _stages(F, M)
    return s_re @ (a_re @ xs) + s_im @ (a_im @ xs), resample_matrix(F, M, smooth)


def error_bound(W, x):
    """2^-23 sum_n |W[m, n]| |x[n, c]|: the fp32 store's half ulp, doubled for the float64 twiddles and sums."""
    return 2.0 ** -23 * (np.abs(W) @ np.abs(np.asarray(x, np.float64)))
