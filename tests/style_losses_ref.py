"""The two style losses restated in numpy from their definitions, with the closed-form gradients the HIP kernels implement
(DESIGN.md 5.19).  Every function takes `dtype`: the float64 run is the truth, the float32 run of the SAME code against it is
the yardstick the tests scale their bounds from (`allowed`).  tests/test_style_losses_cpu.py pins the float64 run, gradients
included, to the reference's recorded outputs and autograd gradients (tests/golden/g14_style_losses.npz).  Nothing here
imports the product.

Style adherence, X (B, T, F) against S (B, K, F):
    d[b, t, k] = mean_f (X[b, t, f] - S[b, k, f])^2
    soft:  w = softmax_k(-lambda d),  L[b, t] = sum_k w_k d_k          hard:  L[b, t] = min_k d_k (lowest index on a tie)
    c[t, k] = w_k (1 - lambda (d_k - L_t))   (soft)     or     [k = argmin]   (hard);   sum_k c[t, k] = 1
    dX[b, t] = (2 / F) g[b, t] sum_k c[t, k] (X[b, t] - S[b, k])
    dS[b, k] = -(2 / F) sum_t g[b, t] c[t, k] (X[b, t] - S[b, k])
NT-Xent, f = cat(a, b) (N = 2 B rows), fhat = f / max(|f|, 1e-12), s = fhat fhat^T / tau, p(i) = (i + B) mod N:
    loss = mean_i [ logsumexp_{j != i} s_ij - s_{i p(i)} ]
    G_ij = up (softmax_{j != i}(s_i)_j - [j = p(i)]) / (N tau),  h = (G + G^T) fhat,
    df_i = (h_i - fhat_i (fhat_i . h_i)) / |f_i|,  or h_i / 1e-12 where |f_i| < 1e-12 (the clamp passes nothing to the norm)."""
import numpy as np

EPS = 1e-12
MARGIN = 8.0          # the project's margin over the float32 yardstick
FLOOR_ULPS = 4.0      # never less than this many fp32 ulps at the tensor's largest magnitude


# ----------------------------------------------------------------------------------------------- style adherence
def distances(X, S, dtype=np.float64):
    X, S = np.asarray(X, dtype), np.asarray(S, dtype)
    diff = X[:, :, None, :] - S[:, None, :, :]
    return (diff * diff).sum(-1) / dtype(X.shape[-1])


def adherence_rows(X, S, lam=10.0, soft=True, dtype=np.float64):
    """-> (L (B, T), c (B, T, K), d (B, T, K)): the rows' loss and the weights both gradients are made of."""
    d = distances(X, S, dtype)
    if soft:
        z = -dtype(lam) * d
        e = np.exp(z - z.max(-1, keepdims=True))
        w = e / e.sum(-1, keepdims=True)
        L = (w * d).sum(-1)
        c = w * (dtype(1) - dtype(lam) * (d - L[..., None]))
    else:
        a = d.argmin(-1)                                   # the first index of the minimum
        L = np.take_along_axis(d, a[..., None], -1)[..., 0]
        c = (np.arange(d.shape[-1]) == a[..., None]).astype(dtype)
    return L.astype(dtype), c, d


def adherence(X, S, lam=10.0, soft=True, reduce=True, dtype=np.float64):
    """The reference's forward: the hard form is the mean whatever `reduce` says."""
    L = adherence_rows(X, S, lam, soft, dtype)[0]
    return L.mean(dtype=dtype) if (reduce or not soft) else L


def adherence_grads(X, S, g, lam=10.0, soft=True, dtype=np.float64):
    """g (B, T): the gradient of the rows (1 / (B T) everywhere for the mean) -> (dX, dS)."""
    X, S, g = np.asarray(X, dtype), np.asarray(S, dtype), np.asarray(g, dtype)
    c = adherence_rows(X, S, lam, soft, dtype)[1]
    gc = g[..., None] * c                                                  # (B, T, K)
    diff = X[:, :, None, :] - S[:, None, :, :]                             # (B, T, K, F)
    two_over_f = dtype(2) / dtype(X.shape[-1])
    dX = two_over_f * (gc[..., None] * diff).sum(2)
    dS = -two_over_f * (gc[..., None] * diff).sum(1)
    return dX.astype(dtype), dS.astype(dtype)


def second_smallest_gap(X, S):
    """min over the rows of (second smallest d - smallest d) / smallest d, in float64: how unambiguous the arg-min is."""
    d = np.sort(distances(X, S), -1)
    return float(((d[..., 1] - d[..., 0]) / d[..., 0]).min()) if d.shape[-1] > 1 else np.inf


# ----------------------------------------------------------------------------------------------- NT-Xent
def _nt_xent_parts(a, b, tau, dtype):
    f = np.concatenate([np.asarray(a, dtype), np.asarray(b, dtype)], 0)
    N = f.shape[0]
    norm = np.sqrt((f * f).sum(1))
    fh = f / np.maximum(norm, dtype(EPS))[:, None]
    s = (fh @ fh.T) / dtype(tau)
    off = ~np.eye(N, dtype=bool)
    m = np.where(off, s, -np.inf).max(1)
    e = np.where(off, np.exp(s - m[:, None]), dtype(0))
    lse = m + np.log(e.sum(1))
    pos = (np.arange(N) + N // 2) % N
    return f, norm, fh, s, off, lse, pos


def nt_xent(a, b, tau, dtype=np.float64):
    _, _, _, s, _, lse, pos = _nt_xent_parts(a, b, tau, dtype)
    return (lse - s[np.arange(s.shape[0]), pos]).mean(dtype=dtype)


def nt_xent_grads(a, b, tau, upstream=1.0, dtype=np.float64):
    """-> (d feature_a, d feature_b)."""
    f, norm, fh, s, off, lse, pos = _nt_xent_parts(a, b, tau, dtype)
    N = f.shape[0]
    P = np.where(off, np.exp(s - lse[:, None]), dtype(0))
    Y = np.zeros_like(P)
    Y[np.arange(N), pos] = 1
    G = dtype(upstream) * (P - Y) / (dtype(N) * dtype(tau))
    h = (G + G.T) @ fh
    proj = h - fh * (fh * h).sum(1, keepdims=True)
    df = np.where((norm >= EPS)[:, None], proj, h) / np.maximum(norm, dtype(EPS))[:, None]
    return df[:N // 2].astype(dtype), df[N // 2:].astype(dtype)


# ----------------------------------------------------------------------------------------------- the bound
def allowed(truth64, run32):
    """The largest absolute error a tensor may have: MARGIN x the float32 run's own distance from the float64 truth, never less
    than FLOOR_ULPS fp32 ulps at the tensor's largest magnitude.  Dividing both sides by max|truth| gives the relative form
    used for the gradient tensors."""
    truth64 = np.asarray(truth64, np.float64)
    yard = float(np.abs(np.asarray(run32, np.float64) - truth64).max())
    floor = FLOOR_ULPS * float(np.spacing(np.float32(np.abs(truth64).max())))
    return max(MARGIN * yard, floor)


def worst(got, truth64):
    return float(np.abs(np.asarray(got, np.float64) - np.asarray(truth64, np.float64)).max())
