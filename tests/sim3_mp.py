"""g2o's Sim3 (sim3.h) and EdgeSim3::computeError at 50 digits (mpmath): the reference the Sim3
unit tests and the pose graph's stage tests hold the device and the float64 NumPy restatement
(essgraph_cases) to.

A Sim3 here is (R, t, s): R a 3 x 3 list of mpf, t a list of 3, s an mpf.  Rows of the C ABI
(q xyzw, t, s as float64) enter through from_row(), which builds R from the quaternion by the
polynomial every implementation uses, exactly, so a float64 row of non-unit length means the same
matrix to all of them.

g2o's branch structure and constants are kept as they stand: both tests against eps = 0.00001 (the
double), R = I + Omega + Omega^2 in the small-angle arm of exp, and the B of the theta ~ 0,
sigma != 0 arm.  log at d = -1 divides by sqrt(1 - d^2) = 0 in g2o itself (NaN): nothing here or
in the tests evaluates it there.

flawed(...) switches deliberate errors on, for the tests that show the bounds discriminate.
"""
import contextlib
import functools

import mpmath as mp
import numpy as np

mp.mp.dps = 50
EPS = mp.mpf(0.00001)    # the double g2o compares with
DELTA = mp.mpf(1e-9)     # the double of g2o's numeric Jacobians
U52 = 2.0 ** -52

FLAWS = ("B_half_small_theta", "B_half_general", "exp_eps_1e-4", "omega_sign", "J_side_swap")
_flaws = set()


@contextlib.contextmanager
def flawed(*names):
    assert all(n in FLAWS for n in names)
    _flaws.update(names)
    try:
        yield
    finally:
        _flaws.difference_update(names)


def _f(x):
    return x if isinstance(x, mp.mpf) else mp.mpf(float(x))


def _skew(w, flaw=False):
    O = [[mp.mpf(0), -w[2], w[1]], [w[2], mp.mpf(0), -w[0]], [-w[1], w[0], mp.mpf(0)]]
    if flaw:
        O[0][1] = w[2]
    return O


def _mm(A, B):
    return [[A[i][0] * B[0][j] + A[i][1] * B[1][j] + A[i][2] * B[2][j] for j in range(3)] for i in range(3)]


def _mv(A, v):
    return [A[i][0] * v[0] + A[i][1] * v[1] + A[i][2] * v[2] for i in range(3)]


def _lin(a, A, b, B, c):
    """a A + b B + c I"""
    return [[a * A[i][j] + b * B[i][j] + (c if i == j else 0) for j in range(3)] for i in range(3)]


def _solve3(W, t):
    """W^-1 t by Cramer's rule (50 digits against a condition number of a few units)"""
    def det(a, b, c):
        return (a[0] * (b[1] * c[2] - b[2] * c[1]) - a[1] * (b[0] * c[2] - b[2] * c[0])
                + a[2] * (b[0] * c[1] - b[1] * c[0]))
    cols = [[W[i][j] for i in range(3)] for j in range(3)]
    D = det(*cols)
    return [det(*[t if k == j else cols[k] for k in range(3)]) / D for j in range(3)]


def _abc(theta, sigma, s, small_theta, eps=EPS):
    """A, B, C of sim3.h's exp (lines 64-146) and log (148-226): the four arms"""
    one = mp.mpf(1)
    small_sigma = abs(sigma) < eps
    C = one if small_sigma else (s - 1) / sigma
    if small_theta:
        if small_sigma:
            return one / 2, one / 6, C
        sigma2 = sigma * sigma
        A = ((sigma - 1) * s + 1) / sigma2
        B = ((sigma2 / 2 - sigma + 1) * s) / (sigma2 * sigma)   # g2o's B, as it stands
        return A, (B / 2 if "B_half_small_theta" in _flaws else B), C
    theta2 = theta * theta
    sn, cs = mp.sin(theta), mp.cos(theta)
    if small_sigma:
        return (1 - cs) / theta2, (theta - sn) / (theta2 * theta), C
    a, b, c = s * sn, s * cs, theta2 + sigma * sigma
    A = (a * sigma + (1 - b) * theta) / (theta * c)
    B = (C - ((b - 1) * sigma + a * theta) / c) / theta2
    return A, (B / 2 if "B_half_general" in _flaws else B), C


def exp(u):
    """g2o::Sim3(const Vector7d&): (omega, upsilon, sigma) -> (R, t, s)"""
    u = [_f(x) for x in u]
    w, ups, sigma = u[:3], u[3:6], u[6]
    theta = mp.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    s = mp.exp(sigma)
    Om = _skew(w, "omega_sign" in _flaws)
    Om2 = _mm(Om, Om)
    eps = mp.mpf(1e-4) if "exp_eps_1e-4" in _flaws else EPS
    small = theta < eps
    A, B, C = _abc(theta, sigma, s, small, eps)
    if small:
        R = _lin(1, Om, 1, Om2, 1)
    else:
        R = _lin(mp.sin(theta) / theta, Om, (1 - mp.cos(theta)) / (theta * theta), Om2, 1)
    return R, _mv(_lin(A, Om, B, Om2, C), ups), s


def exp_generator(u):
    """expm of the 4 x 4 generator [[Omega + sigma I, upsilon], [0, 0]]: (s R, t) of the true
    group exponential, which g2o's general arm equals"""
    u = [_f(x) for x in u]
    Om = _skew(u[:3])
    G = mp.zeros(4)
    for i in range(3):
        for j in range(3):
            G[i, j] = Om[i][j] + (u[6] if i == j else 0)
        G[i, 3] = u[3 + i]
    return mp.expm(G, method="taylor")


def log_d(S):
    """the d = (trace R - 1) / 2 that log tests against 1 - eps"""
    R = S[0]
    return (R[0][0] + R[1][1] + R[2][2] - 1) / 2


def log(S):
    """Sim3::log -> [omega, upsilon, sigma]"""
    R, t, s = S
    sigma = mp.log(s)
    d = log_d(S)
    dR = [R[2][1] - R[1][2], R[0][2] - R[2][0], R[1][0] - R[0][1]]
    near = d > 1 - EPS
    if near:
        theta, k = mp.mpf(0), mp.mpf(1) / 2
    else:
        theta = mp.acos(d)
        k = theta / (2 * mp.sqrt(1 - d * d))
    w = [k * x for x in dR]
    A, B, C = _abc(theta, sigma, s, near)
    Om = _skew(w)
    W = _lin(A, Om, B, _mm(Om, Om), C)
    return w + _solve3(W, t) + [sigma]


def mul(a, b):
    return _mm(a[0], b[0]), [a[2] * x + y for x, y in zip(_mv(a[0], b[1]), a[1])], a[2] * b[2]


def inv(a):
    Rt = [[a[0][j][i] for j in range(3)] for i in range(3)]
    return Rt, [(-1 / a[2]) * x for x in _mv(Rt, a[1])], 1 / a[2]


def smap(a, X):
    return [a[2] * x + y for x, y in zip(_mv(a[0], [_f(v) for v in X]), a[1])]


def edge_error(M, Si, Sj):
    """EdgeSim3::computeError: log(C * v1 * v2^-1)"""
    return log(mul(mul(M, Si), inv(Sj)))


def from_row(row):
    x, y, z, w = (_f(v) for v in row[:4])
    R = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
         [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
         [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
    return R, [_f(v) for v in row[4:7]], _f(row[7])


def quat_from_R(R, sqrt=mp.sqrt):
    """-> ((x, y, z, w), arm): Eigen's matrix -> quaternion, arm 0 for trace > 0, else 1 + the
    index of the largest diagonal entry.  Works on mpf and on floats (sqrt = math.sqrt)."""
    t = R[0][0] + R[1][1] + R[2][2]
    if t > 0:
        r = sqrt(t + 1)
        f = 0.5 / r
        return [(R[2][1] - R[1][2]) * f, (R[0][2] - R[2][0]) * f, (R[1][0] - R[0][1]) * f, r / 2], 0
    i = 0
    if R[1][1] > R[0][0]:
        i = 1
    if R[2][2] > R[i][i]:
        i = 2
    j, k = (i + 1) % 3, (i + 2) % 3
    r = sqrt(R[i][i] - R[j][j] - R[k][k] + 1)
    f = 0.5 / r
    q = [None] * 4
    q[i], q[3] = r / 2, (R[k][j] - R[j][k]) * f
    q[j], q[k] = (R[j][i] + R[i][j]) * f, (R[k][i] + R[i][k]) * f
    return q, 1 + i


def to_row(S):
    """8 mpf: the quaternion of R (quat_from_R), t, s"""
    return quat_from_R(S[0])[0] + list(S[1]) + [S[2]]


def rows_f64(rows_mp):
    return np.array([[float(v) for v in r] for r in rows_mp], np.float64)


def R_rows_f64(R, t, s):
    """float64 (R, t, s) batches -> ABI rows, through the same matrix -> quaternion arms"""
    import math
    out = np.zeros((len(s), 8))
    for i in range(len(s)):
        out[i, :4] = quat_from_R(R[i].tolist(), math.sqrt)[0]
        out[i, 4:7], out[i, 7] = t[i], s[i]
    return out


# ---------------------------------------------------------------- error measures
def _absmax(vals, ref):
    return max(abs(_f(a) - b) for a, b in zip(vals, ref))


def _scaled(vals, ref):
    return _absmax(vals, ref) / max(1, max(abs(b) for b in ref))


def group_errors(kind, out, ref):
    """Largest |out - ref| over a batch per output group.  kind 'sim3' (rows of 8): q up to its
    sign, t scaled by max(1, |t_ref|_inf), s relative; 'log' (rows of 7): omega absolute, upsilon
    scaled by max(1, |upsilon_ref|_inf), sigma absolute; 'point' (rows of 3): scaled like t.
    out: float64 array; ref: rows of mpf.  -> dict group -> float"""
    E = {}

    def put(k, v):
        E[k] = max(E.get(k, 0.0), float(v))
    for o, r in zip(np.asarray(out, np.float64), ref):
        if kind == "sim3":
            put("q", min(_absmax(o[:4], r[:4]), _absmax(-o[:4], r[:4])))
            put("t", _scaled(o[4:7], r[4:7]))
            put("s", abs(_f(o[7]) - r[7]) / abs(r[7]))
        elif kind == "log":
            put("omega", _absmax(o[:3], r[:3]))
            put("upsilon", _scaled(o[3:6], r[3:6]))
            put("sigma", abs(_f(o[6]) - r[6]))
        else:
            put("x", _scaled(o, r))
    return E


def within_bound(E_test, E_64, factor=8.0):
    """the rule of the Sim3 unit and stage tests: E_test <= factor * E_64 + 8 * 2^-52 per group"""
    return all(E_test[k] <= factor * E_64[k] + 8 * U52 for k in E_64)


# ---------------------------------------------------------------- EdgeSim3's numeric Jacobian
def measurements(problem):
    """rows of mpf Sim3: Sjw * Swi from Scw on a loop edge, else from ScwNonCorrected"""
    tabs = [[from_row(r) for r in problem[k]] for k in ("ScwNonCorrected", "Scw")]
    return [mul(tabs[int(l)][j], inv(tabs[int(l)][i]))
            for i, j, l in zip(problem["edge_i"], problem["edge_j"], problem["edge_loop"])]


def linearise(problem, M_rows, est_rows=None):
    """Errors and the exact-arithmetic central differences (delta 1e-9) of EdgeSim3 at the
    estimates est_rows (default Scw) with the float64 measurement rows M_rows (the device's or
    any other: an input here).  oplus is exp(delta e_d) * estimate with the scale entry zeroed under
    bFixScale (which makes column 6 exactly zero); a fixed vertex is skipped (its block stays 0).
    -> err (nE x 7), J (nE x 2 x 7 x 7: [side][row k][column d]) as float64"""
    est = [from_row(r) for r in (problem["Scw"] if est_rows is None else est_rows)]
    ei, ej, fixed, fix = problem["edge_i"], problem["edge_j"], problem["fixed"], bool(problem["bFixScale"])
    nE = len(ei)
    err, J = np.zeros((nE, 7)), np.zeros((nE, 2, 7, 7))
    pert = {}
    for d in range(7):
        for sgn in (1, -1):
            add = [mp.mpf(0)] * 7
            add[d] = sgn * DELTA
            if fix:
                add[6] = mp.mpf(0)
            pert[d, sgn] = exp(add)
    for e in range(nE):
        M, S = from_row(M_rows[e]), (est[ei[e]], est[ej[e]])
        err[e] = [float(v) for v in edge_error(M, S[0], S[1])]
        for side, v in ((0, ei[e]), (1, ej[e])):
            if fixed[v]:
                continue
            for d in range(7):
                ev = []
                for sgn in (1, -1):
                    P = mul(pert[d, sgn], S[side])
                    ev.append(edge_error(M, P, S[1]) if side == 0 else edge_error(M, S[0], P))
                out_side = 1 - side if "J_side_swap" in _flaws else side
                J[e, out_side, :, d] = [float((a - b) / (2 * DELTA)) for a, b in zip(*ev)]
    return err, J


# ---------------------------------------------------------------- input batches of the unit tests
N_ITEMS = 261   # more than one 256-thread block and no multiple of it
PI = float(mp.pi)
THETA = {"T0": 1e-7, "Tbelow": 1e-5 * (1 - 1e-3), "Tabove": 1e-5 * (1 + 1e-3), "T8e-5": 8e-5, "T1e-3": 1e-3,
         "T0.1": 0.1, "T1": 1.0, "T2.5": 2.5, "Tpi": PI - 0.01, "Tlog_in": float(mp.acos(1 - EPS * (1 - mp.mpf(1e-3)))),
         "Tlog_out": float(mp.acos(1 - EPS * (1 + mp.mpf(1e-3))))}
SIGMA = {"S0": 1e-8, "Sbelow": 1e-5 * (1 - 1e-3), "Sabove": 1e-5 * (1 + 1e-3), "S1e-3": 1e-3, "S0.1": 0.1, "S1": 1.0}
# (theta, sigma) classes: every arm at both sides of each threshold (T8e-5 separates a threshold of
# 1e-4 from g2o's 1e-5), the angle sweep, the scale sweep, and d at both sides of log's threshold
EXP_CLASSES = (("T0", "S0"), ("T0", "Sbelow"), ("T0", "Sabove"), ("T0", "S0.1"), ("T0", "S1"),
               ("Tbelow", "Sbelow"), ("Tbelow", "Sabove"), ("Tabove", "Sbelow"), ("Tabove", "Sabove"),
               ("Tbelow", "S0.1"), ("Tabove", "S0.1"), ("T8e-5", "S1e-3"), ("T8e-5", "S0.1"),
               ("T0.1", "S0"), ("T0.1", "Sbelow"), ("T0.1", "Sabove"),
               ("T1e-3", "S0.1"), ("T0.1", "S0.1"), ("T1", "S0.1"), ("T2.5", "S0.1"), ("Tpi", "S0.1"),
               ("T1", "S1e-3"), ("T1", "S1"), ("Tlog_in", "S0.1"), ("Tlog_out", "S0.1"), ("Tlog_in", "S0"),
               ("Tlog_out", "S0"))
AXIS_THETAS = ("T1e-3", "T0.1", "T1", "T2.5", "Tpi")


def _upsilon(rng, n):
    v = rng.standard_normal((n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True) * 10.0 ** rng.uniform(-2, 2, (n, 1))


@functools.lru_cache(maxsize=None)
def exp_inputs():
    """class name -> u (N_ITEMS x 7).  The rotation vector is scaled to the class's angle (to within
    rounding), sigma alternates in sign, |upsilon| is log-uniform in [0.01, 100].  The 'axis' classes
    rotate about +-x, +-y, +-z in turn."""
    out = {}
    for c, (tn, sn) in enumerate(EXP_CLASSES):
        rng = np.random.default_rng(1000 + c)
        w = rng.standard_normal((N_ITEMS, 3))
        w *= THETA[tn] / np.linalg.norm(w, axis=1, keepdims=True)
        sg = SIGMA[sn] * np.where(np.arange(N_ITEMS) % 2, -1.0, 1.0)
        out["%s_%s" % (tn, sn)] = np.concatenate([w, _upsilon(rng, N_ITEMS), sg[:, None]], -1)
    for c, tn in enumerate(AXIS_THETAS):
        rng = np.random.default_rng(2000 + c)
        w = np.zeros((N_ITEMS, 3))
        k = np.arange(N_ITEMS)
        w[k, k % 3] = THETA[tn] * np.where((k // 3) % 2, -1.0, 1.0)
        sg = SIGMA["S0.1"] * np.where(k % 2, -1.0, 1.0)
        out["axis_%s" % tn] = np.concatenate([w, _upsilon(rng, N_ITEMS), sg[:, None]], -1)
    return out


@functools.lru_cache(maxsize=None)
def exp_reference(name):
    """rows of 8 mpf and the matrix -> quaternion arm of each item"""
    S = [exp(u) for u in exp_inputs()[name]]
    return [to_row(s) for s in S], [quat_from_R(s[0])[1] for s in S]


@functools.lru_cache(maxsize=None)
def log_inputs():
    """class name -> rows (N_ITEMS x 8): the float64 roundings of the exp classes' images"""
    return {name: rows_f64(exp_reference(name)[0]) for name in exp_inputs()}


@functools.lru_cache(maxsize=None)
def log_reference(name):
    return [log(from_row(r)) for r in log_inputs()[name]]


def _sim3_rows(rng, n):
    q = rng.standard_normal((n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    t = rng.uniform(-100, 100, (n, 3))
    s = 10.0 ** rng.uniform(-1, 1, (n, 1))
    return np.concatenate([q, t, s], -1)


@functools.lru_cache(maxsize=None)
def group_inputs():
    """mul / inverse / map: scales 0.1 to 10, translations up to 100, points up to 1e3"""
    rng = np.random.default_rng(77)
    return dict(a=_sim3_rows(rng, N_ITEMS), b=_sim3_rows(rng, N_ITEMS), X=rng.uniform(-1e3, 1e3, (N_ITEMS, 3)))


@functools.lru_cache(maxsize=None)
def group_reference(op):
    g = group_inputs()
    a, b = [from_row(r) for r in g["a"]], [from_row(r) for r in g["b"]]
    if op == "mul":
        return [to_row(mul(x, y)) for x, y in zip(a, b)]
    if op == "inverse":
        return [to_row(inv(x)) for x in a]
    return [smap(x, X) for x, X in zip(a, g["X"])]


def threshold_margin(value, threshold=EPS):
    """|value / threshold - 1|: how far (relatively) a branch variable is from its threshold"""
    return abs(value / threshold - 1)


@functools.lru_cache(maxsize=None)
def edge_error_inputs():
    """(M, S_i, S_j) rows of the n12_free ring's edges; M is the float64 quaternion evaluation of
    the measurements (an input like any other)"""
    import essgraph_cases as ec
    pr = ec.ring_case("n12_free")
    M = ec.QuatAlgebra.to_rows(ec.measurements(pr, ec.QuatAlgebra))
    return M, pr["Scw"][pr["edge_i"]], pr["Scw"][pr["edge_j"]]


@functools.lru_cache(maxsize=None)
def edge_error_reference():
    return [edge_error(from_row(m), from_row(a), from_row(b)) for m, a, b in zip(*edge_error_inputs())]


# ---------------------------------------------------------------- the float64 restatement, same inputs
def f64(op, a, b=None, c=None):
    """essgraph_cases' NumPy float64 Sim3 (rotation matrices) on ABI rows -> ABI rows / vectors"""
    import essgraph_cases as ec
    r2s = ec.rows_to_sim3
    if op == "exp":
        return R_rows_f64(*ec.s3_exp(a))
    if op == "log":
        return ec.s3_log(r2s(a))
    if op == "mul":
        return R_rows_f64(*ec.mul(r2s(a), r2s(b)))
    if op == "inverse":
        return R_rows_f64(*ec.inv(r2s(a)))
    if op == "map":
        return ec.smap(r2s(a), np.asarray(b, np.float64))
    assert op == "edge_error"
    return ec.edge_errors(r2s(a), r2s(b), r2s(c), 0)
