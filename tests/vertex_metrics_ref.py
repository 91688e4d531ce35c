"""Float64 restatement of the vertex-space metrics (csrc/vertex_metrics.hip, utils/metrics.py), numpy emulators of
the two kernels' recurrences, the exact truth of the moments in rational arithmetic, the bounds, and the inputs the CPU and GPU
tests share.

BOUNDS.  u = 2^-53 is float64's unit roundoff.

Frame table (restatement against kernel, both in float64 on the exact images of the stored values).  A difference dx carries one
rounding, d2 = (dx dx + dy dy) + dz dz three products and two sums of non-negative terms, sqrt one more: each term is within a few
u relative of its exact value on either side.  A maximum of such terms inherits that: maxima are compared within 8 * 2^-52 relative.
A sum of V non-negative terms adds at most (V - 1) u relative in any order: sums are compared within (V + 8) * 2^-52 relative, twice
the one-sided worst case since both sides round.

Moments.  The kernel runs Welford's recurrence on the computed m^ = m (1 + e), |e| <= 5 u (dx rounds once and enters squared, the
product rounds, two sums round), per frame k = 1 .. n:
    delta = m_k - mean;   mean += delta / k;   M2 += delta * (m_k - mean).
Write B = max_k m_k and R = max_k m_k - min_k m_k of the EXACT m (m >= 0, so R <= B), S = the exact M2.  First order in u:
  mean.  In exact arithmetic mean_k = (1 - 1/k) mean_{k-1} + m_k / k.  The computed step adds e_k m_k / k (|.| <= 5 u B / k) and
    three roundings: delta and the quotient, each scaled by |delta| / k <= R / k, and the sum, scaled by |mean_k| <= B; together
    <= 3 u B.  So err_k <= (1 - 1/k) err_{k-1} + 5 u B / k + 3 u B, and by induction err_k <= 5 u B + 3 k u B <= 8 k u B.
  M2.  Each factor of the product delta * (m_k - mean_k) is at most R in size and is off by at most
    a_k = 5 u B (m_k) + 8 k u B (the mean) + u R (its own rounding); the product rounds once more (u R^2); M2 is a growing sum of
    non-negative terms, so its n additions cost at most n u S.  Summed over k:
       |M2^ - S| <= sum_k (2 R a_k + u R^2) + n u S = u n (R B (8 n + 18) + 3 R^2 + S).
    The factors of the COMPUTED product are bounded by R only up to their own error, so R is replaced by R' = R + 32 n u B; that
    covers data whose spread is of the size of the rounding errors.
  Second-order terms are covered by evaluating both bounds with 2^-52 in place of u (a factor 2; n u << 1 here).
  std = sqrt(M2 / n) then moves by at most |M2^ - S| / (n std) (or sqrt(|M2^ - S| / n) where std = 0), plus two roundings, 2 u std.
The bounds are in terms of R B, not B^2: a variance formed as E[x^2] - E[x]^2, whose error is of order u n B^2, misses them once
B / R is large, which is what the shared moments inputs are made for (B / R of about 10^5)."""
import functools
from fractions import Fraction

import numpy as np

U52 = 2.0 ** -52
THREADS, WAVE = 256, 64


# ----------------------------------------------------------------------------- restatement
def dist2(a, b):
    d = a.astype(np.float64) - b.astype(np.float64)
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def frame_table(pred, gt, lips):
    """(n, 4) float64: max over `lips` of d2, sum of sqrt(d2), max of sqrt(d2), sum of d2 -- numpy's max and sum, NaN and all."""
    with np.errstate(invalid="ignore"):
        d2 = dist2(pred, gt)
        d = np.sqrt(d2)
        return np.stack([np.max(d2[:, np.asarray(lips)], 1), np.sum(d, 1), np.max(d, 1), np.sum(d2, 1)], 1)


def clip_metrics(table, m_pred, m_gt, V):
    """One clip from its rows of the frame table and m (F, U) of both tracks: the definitions of utils/metrics.py."""
    F = table.shape[0]
    return dict(lve=float(np.mean(table[:, 0])), mve=float(np.sum(table[:, 1]) / (F * V)), max_ve=float(np.max(table[:, 2])),
                rmse=float(np.sqrt(np.sum(table[:, 3]) / (F * V))), fdd=float(np.mean(np.std(m_gt, 0)) - np.mean(np.std(m_pred, 0))),
                frames=F)


def metrics(pred, gt, offsets, lips, upper, template):
    """The whole result of utils/metrics.vertex_metrics, restated (two-pass numpy standard deviation)."""
    table = frame_table(pred, gt, lips)
    V, up = pred.shape[1], np.sort(np.asarray(upper))
    clips = []
    for k, (a, b) in enumerate(zip(offsets[:-1], offsets[1:])):
        t = template if template.ndim == 2 else template[k]
        clips.append(clip_metrics(table[a:b], dist2(pred[a:b][:, up], t[up]), dist2(gt[a:b][:, up], t[up]), V))
    n = offsets[-1]
    pooled = dict(lve=float(np.mean(table[:, 0])), mve=float(np.sum(table[:, 1]) / (n * V)), max_ve=float(np.max(table[:, 2])),
                  rmse=float(np.sqrt(np.sum(table[:, 3]) / (n * V))), fdd=float(np.mean([c["fdd"] for c in clips])), frames=n)
    return {"clips": clips, "all": pooled}


def table_ok(got, want, V):
    """Columns 0 / 2 within 8 * 2^-52, columns 1 / 3 within (V + 8) * 2^-52, relative; NaN where and only where the restatement has it.
    -> (ok, worst error / bound)."""
    tol = np.array([8, V + 8, 8, V + 8]) * U52 * np.abs(want)
    nan = np.isnan(want)
    if not np.array_equal(nan, np.isnan(got)):
        return False, np.inf
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.where(nan | (got == want), 0.0, np.abs(got - want))
        worst = float(np.max(np.where(err > 0, err / np.maximum(tol, 1e-300), 0.0), initial=0.0))
        return bool((nan | (err <= tol)).all()), worst


# ----------------------------------------------------------------------------- emulator of the frame kernel
def nan_max(a, b):
    return np.where((b > a) | (b != b), b, a)


def emulate_frame_table(pred, gt, region, vmax=nan_max, lip_all=False):
    """The kernel's own order in numpy float64: thread t folds vertices t, t + 256, ..., a wave joins by the xor butterfly, the four
    waves join in order.  vmax = np.fmax plants the NaN-dropping maximum; lip_all takes column 0 over every vertex."""
    n, V = pred.shape[:2]
    with np.errstate(invalid="ignore"):
        d2 = dist2(pred, gt)
        d = np.sqrt(d2)
        lip = np.ones(V, bool) if lip_all else (np.asarray(region) & 1).astype(bool)
        acc = [np.zeros((n, THREADS)) for _ in range(4)]
        for v0 in range(0, V, THREADS):
            w = min(THREADS, V - v0)
            s = slice(v0, v0 + w)
            acc[0][:, :w] = np.where(lip[s], vmax(acc[0][:, :w], d2[:, s]), acc[0][:, :w])
            acc[1][:, :w] = acc[1][:, :w] + d[:, s]
            acc[2][:, :w] = vmax(acc[2][:, :w], d[:, s])
            acc[3][:, :w] = acc[3][:, :w] + d2[:, s]
        join = lambda a, b: [vmax(a[0], b[0]), a[1] + b[1], vmax(a[2], b[2]), a[3] + b[3]]
        lane = np.arange(THREADS)
        for o in (32, 16, 8, 4, 2, 1):
            acc = join(acc, [x[:, lane ^ o] for x in acc])
        r = [x[:, 0] for x in acc]
        for w in range(1, THREADS // WAVE):
            r = join(r, [x[:, w * WAVE] for x in acc])
    return np.stack(r, 1)


# ----------------------------------------------------------------------------- moments: emulator, exact truth, bounds
def emulate_moments(pred, gt, offsets, upper_idx, template, mode="welford"):
    """state (n_clips, U, 2, 3) = [pred | gt][count, mean, M2] by the kernel's recurrence, frame by frame in float64.  upper_idx is
    clamped into [0, V) as the kernel clamps it.  Planted mutants: mode 'fp32' keeps the state in fp32, 'unshifted' forms
    M2 = sum m^2 - (sum m)^2 / n."""
    V = pred.shape[1]
    up = np.clip(np.asarray(upper_idx, np.int64), 0, V - 1)
    acc = np.float32 if mode == "fp32" else np.float64
    state = np.zeros((len(offsets) - 1, len(up), 2, 3))
    for k, (a, b) in enumerate(zip(offsets[:-1], offsets[1:])):
        t = (template if template.ndim == 2 else template[k])[up]
        for j, x in enumerate((pred, gt)):
            cnt, mean, m2, s1 = acc(0), np.zeros(len(up), acc), np.zeros(len(up), acc), np.zeros(len(up), acc)
            for f in range(a, b):
                m = dist2(x[f, up], t).astype(acc)
                cnt = acc(cnt + acc(1))
                if mode == "unshifted":
                    s1 = s1 + m
                    m2 = m2 + m * m
                else:
                    delta = m - mean
                    mean = mean + delta / cnt
                    m2 = m2 + delta * (m - mean)
            if mode == "unshifted":
                mean, m2 = s1 / cnt, m2 - s1 * s1 / cnt
            state[k, :, j, 0], state[k, :, j, 1], state[k, :, j, 2] = cnt, mean, m2
    return state


def state_std(state, sample=False):
    """(n_clips, U, 2) standard deviation of m from a state; sample = True plants the n - 1 divisor (a one-frame clip stays 0)."""
    n = state[..., 0]
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.sqrt(np.where(n > 1, state[..., 2] / (n - 1 if sample else n), 0.0))


def exact_moments(pred, gt, offsets, upper_idx, template):
    """Per (clip, u, track): (n, mean, S, B, R) as Fractions from the stored values, which are binary floats and hence rationals."""
    V = pred.shape[1]
    up = np.clip(np.asarray(upper_idx, np.int64), 0, V - 1)
    out = []
    for k, (a, b) in enumerate(zip(offsets[:-1], offsets[1:])):
        t = (template if template.ndim == 2 else template[k])[up].astype(np.float64)
        rows = []
        for i in range(len(up)):
            tf = [Fraction(float(c)) for c in t[i]]
            pair = []
            for x in (pred, gt):
                xs = x[a:b, up[i]].astype(np.float64)
                m = [sum((Fraction(float(c)) - tc) ** 2 for c, tc in zip(row, tf)) for row in xs]
                n = len(m)
                s1 = sum(m)
                pair.append((n, s1 / n, sum(v * v for v in m) - s1 * s1 / n, max(m), max(m) - min(m)))
            rows.append(pair)
        out.append(rows)
    return out


def moment_bounds(n, S, B, R):
    """(mean bound, M2 bound) of the module docstring, floats, a hair above the rational value."""
    B, R, S = float(B) * (1 + 1e-12), float(R) * (1 + 1e-12), float(S) * (1 + 1e-12)
    Rp = R + 32 * n * U52 * B
    return 8 * n * U52 * B, U52 * n * (Rp * B * (8 * n + 18) + 3 * Rp * Rp + S)


def std_bound(n, S, B, R):
    """Bound on |sqrt(M2^ / n) - sqrt(S / n)|."""
    b = moment_bounds(n, S, B, R)[1] / n
    std = float(S / n) ** 0.5
    return (min(b ** 0.5, b / std) if std > 0 else b ** 0.5) + 2 * U52 * std


def check_state(state, exact):
    """-> (ok, worst error / bound over count, mean and M2) of a state against `exact_moments`."""
    ok, worst = True, 0.0
    for k, rows in enumerate(exact):
        for i, pair in enumerate(rows):
            for j, (n, mean, S, B, R) in enumerate(pair):
                bm, bs = moment_bounds(n, S, B, R)
                cnt, gm, gs = (float(x) for x in state[k, i, j])
                if cnt != n or not (np.isfinite(gm) and np.isfinite(gs)):
                    return False, np.inf
                em, es = float(abs(Fraction(gm) - mean)), float(abs(Fraction(gs) - S))
                ok &= em <= bm and es <= bs
                worst = max(worst, em / bm if bm else float(em > 0) * np.inf, es / bs if bs else float(es > 0) * np.inf)
    return ok, worst


def check_std(std, exact):
    """-> (ok, worst error / bound) of (n_clips, U, 2) standard deviations against the exact ones."""
    ok, worst = True, 0.0
    for k, rows in enumerate(exact):
        for i, pair in enumerate(rows):
            for j, (n, mean, S, B, R) in enumerate(pair):
                b = std_bound(n, S, B, R)
                e = abs(float(std[k, i, j]) - float(S / n) ** 0.5)
                if not e <= b:
                    ok = False
                worst = max(worst, e / b if b else float(e > 0) * np.inf)
    return ok, worst


def fdd_exact_and_bound(exact):
    """Per clip: (fdd from the exact moments, the bound on a computed fdd: the std bounds averaged, plus the two means' and the
    difference's roundings)."""
    out = []
    for rows in exact:
        sp = [float(p[0][2] / p[0][0]) ** 0.5 for p in rows]
        sg = [float(p[1][2] / p[1][0]) ** 0.5 for p in rows]
        b = sum(std_bound(*p[0][0:1], *p[0][2:]) + std_bound(*p[1][0:1], *p[1][2:]) for p in rows) / len(rows)
        out.append((float(np.mean(sg) - np.mean(sp)), b + 4 * U52 * (np.mean(sg) + np.mean(sp))))
    return out


# ----------------------------------------------------------------------------- shared inputs
FRAME_V = (1, 63, 64, 65, 255, 256, 257, 5023)
LIP_MASKS = ("first", "last", "all", "third")


def lip_mask(kind, V):
    return {"first": np.array([0]), "last": np.array([V - 1]), "all": np.arange(V), "third": np.arange(0, V, 3)}[kind]


@functools.lru_cache(maxsize=None)
def frame_case(V, n, half, kind, plant):
    """(pred, gt, lips, region): n frames of V vertices, fp16 if half.  plant = 'first' / 'last' puts the frame's largest error at
    vertex 0 / V - 1; frame f plants it there (f even) or leaves that vertex out of the lips where the mask allows, so that columns
    0 and 2 differ on masks that do not hold the planted vertex."""
    g = np.random.default_rng(1000 * V + 10 * n + 2 * half + LIP_MASKS.index(kind) * 7 + (plant == "last"))
    dt = np.float16 if half else np.float32
    gt = (0.1 * g.standard_normal((n, V, 3))).astype(dt)
    pred = (gt.astype(np.float64) + 0.01 * g.standard_normal((n, V, 3))).astype(dt)
    at = 0 if plant == "first" else V - 1
    pred[:, at] = (gt[:, at].astype(np.float64) + np.array([0.5, -0.25, 0.125])).astype(dt)
    lips = lip_mask(kind, V)
    region = np.zeros(V, np.uint8)
    region[lips] |= 1
    region[np.arange(0, V, 2)] |= 2
    return pred, gt, lips, region


MOMENT_CLIPS = (0, 5, 7, 40, 41)        # clips of 5, 2, 33 and 1 frames: chunks of 7 cut inside a clip and exactly at offset 7
MOMENT_V = 331
MOMENT_U = (1, 63, 64, 65, 300)


@functools.lru_cache(maxsize=None)
def moments_case(U, per_clip, half=False):
    """(pred, gt, upper_idx, template): 41 frames of 331 vertices, each track a large constant offset from the template plus motion
    of 2^-14 steps -- mean of m about 10^5 times its spread."""
    g = np.random.default_rng(77 + U + 1000 * per_clip + 5000 * half)
    n, V = MOMENT_CLIPS[-1], MOMENT_V
    dt = np.float16 if half else np.float32
    step = 2.0 ** -5 if half else 2.0 ** -14
    template = (0.1 * g.standard_normal((4, V, 3) if per_clip else (V, 3))).astype(np.float32)
    base = template if not per_clip else np.repeat(template, np.diff(MOMENT_CLIPS), axis=0)
    mk = lambda off: (base + np.asarray(off) + step * g.integers(-8, 9, (n, V, 3))).astype(dt)
    pred, gt = mk([40.0, -25.0, 10.0]), mk([39.0, -26.0, 11.0])
    upper = np.sort(g.choice(V, U, replace=False)).astype(np.int32)
    return pred, gt, upper, template


@functools.lru_cache(maxsize=None)
def moments_exact_case(U, per_clip, half=False):
    pred, gt, upper, template = moments_case(U, per_clip, half)
    return exact_moments(pred, gt, list(MOMENT_CLIPS), upper, template)
