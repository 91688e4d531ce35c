"""The numpy truth of the audio front end (include/msmd_hip.h): downmix, the Kaiser-windowed sinc evaluated
DIRECTLY (no table), z-normalisation.  float64 is the truth; the same code with float32 taps, products and sums is the
yardstick the GPU bounds are stated against.  Nothing here is imported by the product."""
import math

import numpy as np

FS_OUT = 16000
ZEROS = 64
BETA = 14.769656459379492
ROLLOFF = 0.9475937167399596


def ratio(fs_in, fs_out=FS_OUT):
    g = math.gcd(int(fs_in), int(fs_out))
    return fs_out // g, fs_in // g           # L, M


def h(t, L, M):
    """The filter at t input samples, float64."""
    s = ROLLOFF * min(1.0, L / M)
    u = s * np.asarray(t, np.float64)
    inside = np.abs(u) < ZEROS
    arg = np.where(inside, 1.0 - (u / ZEROS) ** 2, 0.0)
    return np.where(inside, s * np.sinc(u) * np.i0(BETA * np.sqrt(arg)) / np.i0(BETA), 0.0)


def downmix_ref(pcm, dtype=np.float64):
    """pcm (frames, channels) or 1-D, int16 or float32 -> mono: channels summed in order, divided by their number; int16
    scaled by 2^-15 first."""
    a = np.asarray(pcm)
    if a.ndim == 1:
        a = a[:, None]
    x = a.astype(dtype) * dtype(2.0 ** -15) if a.dtype == np.int16 else a.astype(dtype)
    acc = np.zeros(a.shape[0], dtype)
    for c in range(a.shape[1]):
        acc = acc + x[:, c]
    return acc / dtype(a.shape[1])


def out_len(n, L, M):
    return -((-n * L) // M)


def resample_ref(x, fs_in, dtype=np.float64):
    """y[n] = sum_k x[k] h(n M / L - k), n < ceil(N L / M), x zero outside [0, N).  The sum runs over k ascending from
    n M div L - W to n M div L + W + 1, W = ceil(64 / s), which holds every non-zero tap; t = (n M - k L) / L is formed from
    the exact integer numerator.  dtype float32: taps rounded to float32, products and the running sum in float32."""
    x = np.asarray(x, dtype)
    L, M = ratio(fs_in)
    if L == M:
        return x.copy()
    N = x.shape[0]
    n = np.arange(out_len(N, L, M), dtype=np.int64)
    s = ROLLOFF * min(1.0, L / M)
    W = math.ceil(ZEROS / s)
    k0 = (n * M) // L
    acc = np.zeros(n.shape[0], dtype)
    for j in range(-W, W + 2):
        k = k0 + j
        ok = (k >= 0) & (k < N)
        tap = h((n * M - k * L).astype(np.float64) / L, L, M).astype(dtype)
        acc = acc + np.where(ok, x[np.clip(k, 0, N - 1)], dtype(0)) * tap
    return acc


def znorm_ref(y, dtype=np.float64):
    y = np.asarray(y, dtype)
    return (y - y.mean(dtype=dtype)) / (y.std(dtype=dtype) + dtype(1e-5))
