"""Numpy restatement of the expression fit (include/msmd_hip.h): test infrastructure.

The landmarks come through the FULL FLAME path -- blend shapes, pose correctives and linear blend skinning over every vertex
(tests/test_geometry_gpu.py::lbs64's recipe, here at any dtype), then the barycentric lookup -- not through the reduced tables
the kernel reads.  The Jacobian is analytic, the Levenberg-Marquardt loop is the one the header states.  dtype= runs the same
code in float32."""
import numpy as np

J, JAW = 5, 2
PARENTS = np.array([-1, 0, 1, 1, 1])


def model_from_asset(asset, n_shape=100, n_exp=50):
    """The arrays of a FLAME asset dict as utils/flame.FLAME keeps them (fp32 values), with n_exp expression directions."""
    sd = np.asarray(asset["shapedirs"], np.float32)
    V = sd.shape[0]
    return dict(v_template=np.asarray(asset["v_template"], np.float32),
                shapedirs=np.concatenate([sd[:, :, :n_shape], sd[:, :, 300:300 + n_exp]], 2),
                posedirs=np.asarray(asset["posedirs"], np.float32).reshape(V * 3, -1).T.copy(),
                J_regressor=np.asarray(asset["J_regressor"], np.float32), weights=np.asarray(asset["weights"], np.float32),
                faces=np.asarray(asset["f"]).astype(np.int64), n_shape=n_shape, n_exp=n_exp)


def rodrigues(r, dtype=np.float64):
    """utils/lbs.py's convention: angle = |r + 1e-8|, direction = r / angle.  (N, 3) -> (N, 3, 3)."""
    r = np.asarray(r, dtype)
    angle = np.sqrt(((r + dtype(1e-8)) ** 2).sum(1, keepdims=True))
    d = r / angle
    s, c = np.sin(angle)[:, None], np.cos(angle)[:, None]
    z = np.zeros_like(d[:, 0])
    K = np.stack([z, -d[:, 2], d[:, 1], d[:, 2], z, -d[:, 0], -d[:, 1], d[:, 0], z], 1).reshape(-1, 3, 3)
    return np.eye(3, dtype=dtype)[None] + s * K + (1 - c) * (K @ K)


def rodrigues_jet(th, dtype=np.float64):
    """th (3) -> (M = R - I (3, 3), dR (3, 3, 3) with dR[a] = d R / d th_a), analytic."""
    th = np.asarray(th, dtype)
    t = th + dtype(1e-8)
    al = np.sqrt((t * t).sum())
    d = th / al
    skew = lambda v: np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], dtype)
    K = skew(d)
    K2 = K @ K
    s, co = np.sin(al), np.cos(al)
    c1 = 2 * np.sin(al / 2) ** 2
    M = s * K + c1 * K2
    dR = np.empty((3, 3, 3), dtype)
    for a in range(3):
        aa = t[a] / al
        dd = np.eye(3, dtype=dtype)[a] / al - th * aa / (al * al)
        Ka = skew(dd)
        dR[a] = co * aa * K + s * Ka + s * aa * K2 + c1 * (Ka @ K + K @ Ka)
    return M.astype(dtype), dR


def lbs_full(m, betas, pose, dtype=np.float64):
    """utils/lbs.py:141-223 at `dtype` over every vertex: betas (B, n_shape + n_exp), pose (B, 15) -> verts (B, V, 3)."""
    f = lambda x: np.asarray(x, dtype)
    betas = f(betas)
    B, NB = betas.shape
    V = m["v_template"].shape[0]
    v_shaped = f(m["v_template"])[None] + (betas @ f(m["shapedirs"]).reshape(V * 3, NB).T).reshape(B, V, 3)
    joints = np.einsum("jv,bvc->bjc", f(m["J_regressor"]), v_shaped)
    R = rodrigues(f(pose).reshape(B * J, 3), dtype).reshape(B, J, 3, 3)
    pf = (R[:, 1:] - np.eye(3, dtype=dtype)).reshape(B, (J - 1) * 9)
    p = v_shaped + (pf @ f(m["posedirs"])).reshape(B, V, 3)
    wR, wt = [R[:, 0]], [joints[:, 0]]
    for i in range(1, J):
        pa = PARENTS[i]
        wR.append(wR[pa] @ R[:, i])
        wt.append(np.einsum("brc,bc->br", wR[pa], joints[:, i] - joints[:, pa]) + wt[pa])
    A = np.stack([np.concatenate([wR[i], (wt[i] - np.einsum("brc,bc->br", wR[i], joints[:, i]))[:, :, None]], 2) for i in range(J)], 1)
    T = np.einsum("vj,bjk->bvk", f(m["weights"]), A.reshape(B, J, 12)).reshape(B, V, 3, 4)
    return np.einsum("bvrc,bvc->bvr", T[..., :3], p) + T[..., 3]


def landmarks_full(m, fidx, bary, shape, e, theta, dtype=np.float64):
    """FLAME.forward(shape, e, [0, 0, 0, theta]) -> vertices2landmarks: shape (B, n_shape), e (B, NE), theta (B, 3) -> (B, K, 3)."""
    e, theta = np.asarray(e, dtype), np.asarray(theta, dtype)
    B = e.shape[0]
    pose = np.zeros((B, 15), dtype)
    pose[:, 6:9] = theta
    v = lbs_full(m, np.concatenate([np.broadcast_to(np.asarray(shape, dtype), (B, m["n_shape"])), e], 1), pose, dtype)
    vidx = m["faces"][np.asarray(fidx).reshape(-1)]
    return np.einsum("bkcx,kc->bkx", v[:, vidx], np.asarray(bary, dtype).reshape(-1, 3))


def jacobian(m, fidx, bary, shape, e, theta, dtype=np.float64):
    """d l_k / d [e | theta] at one frame, analytic: -> (K, 3, NE + 3).  From the model's arrays at the landmarks' corner
    vertices: v = s x + w (R - I)(x - J), x = template + S beta + E e + P vec(R - I), J the jaw joint of the shaped template."""
    f = lambda x: np.asarray(x, dtype)
    ns, NE = m["n_shape"], m["n_exp"]
    V = m["v_template"].shape[0]
    vidx = m["faces"][np.asarray(fidx).reshape(-1)]                       # (K, 3)
    bary = f(bary).reshape(-1, 3)
    sd = f(m["shapedirs"])
    betas = np.concatenate([f(shape).reshape(-1), f(e)])
    M, dR = rodrigues_jet(theta, dtype)
    P = f(m["posedirs"])[9 * (JAW - 1):9 * JAW].reshape(9, V, 3)
    x = f(m["v_template"])[vidx] + sd[vidx] @ betas + np.einsum("mkcx,m->kcx", P[:, vidx], M.reshape(9))
    jr = f(m["J_regressor"])[JAW]
    Jj = jr @ (f(m["v_template"]) + sd @ betas)
    JE = np.einsum("v,vxl->xl", jr, sd[:, :, ns:])
    s, w = f(m["weights"])[vidx].sum(-1), f(m["weights"])[vidx, JAW]      # (K, 3)
    E = sd[vidx][..., ns:]                                                # (K, 3, 3, NE)
    de = s[..., None, None] * E + w[..., None, None] * np.einsum("xy,kcyl->kcxl", M, E - JE)
    Pq = np.einsum("mkcx,am->kcxa", P[:, vidx], dR.reshape(3, 9))         # P d vec(R) / d theta_a
    dt = s[..., None, None] * Pq + w[..., None, None] * (np.einsum("axy,kcy->kcxa", dR, x - Jj) + np.einsum("xy,kcya->kcxa", M, Pq))
    return np.einsum("kc,kcxp->kxp", bary, np.concatenate([de, dt], -1))


def free_columns(NE, jaw_dof):
    return list(range(NE)) + [NE + a for a in range(jaw_dof)]


def fit(m, fidx, bary, shapes, subject, y, w=None, jaw_dof=1, lambda_exp=1e-6, lambda_jaw=0.0, iterations=12, dtype=np.float64):
    """The solver of include/msmd_hip.h, frame by frame.  shapes (S, n_shape), subject (n) ints (clamped), y (n, K, 3).
    -> dict: hist (iterations + 1, n, NE + 3) the iterate [e | theta] after 0, 1, ... iterations, code (n, NE), jaw (n, 3),
    rms (n), status (n) int32, as the kernel returns them but at `dtype`."""
    y = np.asarray(y)
    n, K = y.shape[:2]
    NE = m["n_exp"]
    w = np.ones(K, dtype) if w is None else np.asarray(w, dtype)
    shapes = np.asarray(shapes, dtype).reshape(-1, m["n_shape"])
    free = free_columns(NE, jaw_dof)
    D = np.array([lambda_exp] * NE + [lambda_jaw] * jaw_dof, dtype)
    sw = np.sqrt(w)
    hist = np.zeros((iterations + 1, n, NE + 3), dtype)
    rms, status = np.zeros(n, dtype), np.zeros(n, np.int32)
    for i in range(n):
        shape = shapes[min(max(int(subject[i]), 0), len(shapes) - 1)][None]
        yi = y[i].astype(dtype)
        if not np.all(np.isfinite(y[i])):
            hist[:, i], rms[i], status[i] = np.nan, np.nan, 1
            continue

        def residual(pfull):
            return landmarks_full(m, fidx, bary, shape, pfull[None, :NE], pfull[None, NE:], dtype)[0] - yi

        def objective(pfull):
            r = residual(pfull)
            fd = ((sw[:, None] * r) ** 2).sum()
            return fd + (D * pfull[free] ** 2).sum(), fd
        p = np.zeros(NE + 3, dtype)
        mu = dtype(1e-3)
        fcur, fdata = objective(p)
        for it in range(iterations):
            r = residual(p)
            Jm = jacobian(m, fidx, bary, shape, p[:NE], p[NE:], dtype)[:, :, free]
            Js = (sw[:, None, None] * Jm).reshape(K * 3, len(free))
            rs = (sw[:, None] * r).reshape(K * 3)
            H = Js.T @ Js + np.diag(D)
            g = Js.T @ rs + D * p[free]
            A = H + mu * np.diag(np.diag(H))
            ok = True
            try:
                Lc = np.linalg.cholesky(A)
                delta = -np.linalg.solve(Lc.T, np.linalg.solve(Lc, g))
            except np.linalg.LinAlgError:
                ok = False
                status[i] |= 2
            if ok:
                pt = p.copy()
                pt[free] = p[free] + delta
                ft, fdt = objective(pt)
                ok = bool(ft <= fcur)
            if ok:
                p, fcur, fdata = pt, ft, fdt
                mu = max(mu / dtype(10), dtype(1e-9))
            else:
                mu = mu * dtype(10)
            hist[it + 1, i] = p
        rms[i] = np.sqrt(fdata / w.sum())
    return dict(hist=hist, code=hist[-1, :, :NE], jaw=hist[-1, :, NE:], rms=rms, status=status)


def reduce_tables(m, fidx, bary, shapes):
    """The numpy twin of utils/expression_fit.reduce_flame, float64: (tab (K, 6, NE + 9), tab0 (S, K, 6))."""
    f = lambda x: np.asarray(x, np.float64)
    ns, NE = m["n_shape"], m["n_exp"]
    V = m["v_template"].shape[0]
    vidx = m["faces"][np.asarray(fidx).reshape(-1)]
    bary = f(bary).reshape(-1, 3)
    sd, jr, wt = f(m["shapedirs"]), f(m["J_regressor"])[JAW], f(m["weights"])
    P = f(m["posedirs"])[9 * (JAW - 1):9 * JAW].reshape(9, V, 3)
    vs = f(m["v_template"])[None] + np.einsum("vcl,sl->svc", sd[:, :, :ns], f(shapes).reshape(-1, ns))
    bs, bw = bary * wt[vidx].sum(-1), bary * wt[vidx, JAW]
    E, Pc = sd[vidx][..., ns:], np.transpose(P[:, vidx], (1, 2, 3, 0))
    JE, J0 = np.einsum("v,vcl->cl", jr, sd[:, :, ns:]), np.einsum("v,svc->sc", jr, vs)
    tab = np.concatenate([np.concatenate([np.einsum("kc,kcxl->kxl", bs, E), np.einsum("kc,kcxl->kxl", bs, Pc)], 2),
                          np.concatenate([np.einsum("kc,kcxl->kxl", bw, E - JE), np.einsum("kc,kcxl->kxl", bw, Pc)], 2)], 1)
    x0 = vs[:, vidx]
    tab0 = np.concatenate([np.einsum("kc,skcx->skx", bs, x0), np.einsum("kc,skcx->skx", bw, x0 - J0[:, None, None])], 2)
    return tab, tab0


def landmarks_reduced(tab, tab0, s, e, theta):
    """l = X + M Y from the reduced tables at one frame: -> (K, 3)."""
    M, _ = rodrigues_jet(theta)
    v = tab0[s] + tab @ np.concatenate([np.asarray(e, np.float64), M.reshape(9)])
    return v[:, :3] + v[:, 3:] @ M.T


# ----------------------------------------------------------------------------- the cases the CPU and GPU tests share
def embedding(K, n_faces, tag="expfit"):
    """K landmarks on random faces with random barycentric weights (seeded by K)."""
    g = np.random.default_rng(1000 + K)
    b = g.random((K, 3)) + 0.05
    return g.integers(0, n_faces, K), (b / b.sum(1, keepdims=True)).astype(np.float32)


def case_inputs(m, K, n, S, seed, theta=(0.5, 0.1, -0.08), noise=2e-4, exp_scale=1.5):
    """Synthetic targets: e ~ exp_scale N(0, 1), the given jaw pose (a little different per frame), noise,
    weights in [0.5, 2] with every seventh zero, subjects interleaved frame by frame.  -> dict."""
    g = np.random.default_rng(seed)
    fidx, bary = embedding(K, m["faces"].shape[0])
    shapes = 0.5 * g.standard_normal((S, m["n_shape"]))
    shapes = shapes.astype(np.float32).astype(np.float64)
    subject = (np.arange(n) % S).astype(np.int32)
    e = exp_scale * g.standard_normal((n, m["n_exp"]))
    th = np.asarray(theta, np.float64)[None] * (1.0 + 0.1 * g.standard_normal((n, 1)))
    y = np.stack([landmarks_full(m, fidx, bary, shapes[subject[i]][None], e[i:i + 1], th[i:i + 1])[0] for i in range(n)])
    y = (y + noise * g.standard_normal(y.shape)).astype(np.float32)
    w = g.uniform(0.5, 2.0, K)
    w[::7] = 0.0
    if K < 7:
        w[:] = g.uniform(0.5, 2.0, K)
    return dict(fidx=fidx, bary=bary, shapes=shapes, subject=subject, e=e, theta=th, y=y, w=w)


# name: K, NE, jaw_dof, n frames (the first D of them distinct, then repeated), S, iterations, lambda_exp, lambda_jaw, theta, noise.
# 12 iterations and the default prior wherever the float64 run sits still by then (tests/test_expression_fit_cpu.py checks
# |iterate(N - 4) - iterate(N)| < 2^-26 max(1, |p|) for every row).  Measured on the synthetic asset: K = 18 needs 32 iterations
# with jaw_dof 1 and 48 with jaw_dof 3; one landmark with a free jaw (3 equations, 51 .. 53 unknowns) needs the prior at 1e-2 on
# both blocks and 64 iterations.  n runs over 1, 2, FRAMES - 1, FRAMES, FRAMES + 1 and 257 (FRAMES = 4 frames per workgroup).
FRAMES = 4
DEF = dict(NE=50, n=FRAMES + 1, D=3, S=1, its=12, le=1e-6, lj=0.0, theta=(0.5, 0.1, -0.08), noise=2e-4)
CASES = {}
for _K in (1, 18, 51, 68, 105, 128):
    for _jd in (0, 1, 3):
        _c = dict(DEF, K=_K, jd=_jd)
        if _K == 18 and _jd:
            _c["its"] = 32 if _jd == 1 else 48
        if _K == 1 and _jd:
            _c.update(its=64, le=1e-2, lj=1e-2, D=2)
        CASES[f"K{_K}-jaw{_jd}"] = _c
for _NE in (1, 61):
    for _jd in (1, 3):
        CASES[f"NE{_NE}-jaw{_jd}"] = dict(DEF, K=68, NE=_NE, jd=_jd, n=2, D=2)
for _n in (1, 2, FRAMES - 1, FRAMES, 257):
    CASES[f"n{_n}"] = dict(DEF, K=51, jd=1, n=_n, D=min(_n, 8))
CASES["subjects3"] = dict(DEF, K=68, jd=1, n=2 * FRAMES - 1, D=6, S=3)
CASES["iterations0"] = dict(DEF, K=68, jd=1, n=2, D=2, its=0)
CASES["theta0"] = dict(DEF, K=68, jd=3, n=2, D=2, theta=(0.0, 0.0, 0.0), noise=0.0)

_MODELS, _REFS = {}, {}


def model(NE):
    if NE not in _MODELS:
        from msmd_amd import synth
        _MODELS[NE] = model_from_asset(synth.flame_asset(), 100, NE)
    return _MODELS[NE]


def reference(name):
    """One case's inputs and float64 run, computed once per session: the inputs (n frames), the restatement's iterate after
    `its` iterations (p), its floor max |iterate(its) - iterate(its + 4)|, its rms, and still = max |iterate(its - 4) -
    iterate(its)| (None below 4 iterations)."""
    if name in _REFS:
        return _REFS[name]
    import zlib
    c = CASES[name]
    m = model(c["NE"])
    inp = case_inputs(m, c["K"], c["D"], c["S"], zlib.crc32(name.encode()) % 10000, c["theta"], c["noise"])
    its = c["its"]
    extra = 4 if its else 0
    r = fit(m, inp["fidx"], inp["bary"], inp["shapes"], inp["subject"], inp["y"], inp["w"], c["jd"], c["le"], c["lj"], its + extra)
    h = r["hist"]
    rep = np.arange(c["n"]) % c["D"]
    out = dict(c, m=m, fidx=inp["fidx"], bary=inp["bary"], shapes=inp["shapes"], w=inp["w"], y=inp["y"][rep],
               subject=inp["subject"][rep], p=h[its][rep], floor=float(np.abs(h[its] - h[its + extra]).max()),
               still=float(np.abs(h[its] - h[its - 4]).max()) if its >= 4 else None, status=r["status"][rep])
    if its:
        r0 = fit(m, inp["fidx"], inp["bary"], inp["shapes"], inp["subject"], inp["y"], inp["w"], c["jd"], c["le"], c["lj"], its)
        assert np.array_equal(r0["hist"][its], h[its])
        out["rms"] = r0["rms"][rep]
    else:
        out["rms"] = r["rms"][rep]
    _REFS[name] = out
    return out
