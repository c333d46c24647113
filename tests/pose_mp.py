"""g2o's SE3Quat (se3quat.h), EdgeSE3ProjectXYZOnlyPose / EdgeStereoSE3ProjectXYZOnlyPose
(types_six_dof_expmap.cpp) with RobustKernelHuber, and the 28 terms of PoseOptimization's 6 x 6
system, at 50 digits (mpmath): the reference the SE3 unit tests and the pose stage tests hold the
device and the float64 NumPy restatement below to.  Written from the definitions, not from the
oracle (oracle/ba.c) or the kernel.

An SE3 here is (R, t): R a 3 x 3 list of mpf, t a list of 3.  Rows of the C ABI (q xyzw, t as
float64) enter through from_row(), which builds R from the quaternion by the polynomial every
implementation uses, exactly.

Kept as g2o and the reference have them: exp's test against the double 0.00001 with
R = V = I + Omega + Omega^2 below it (truncation included; SE3Quat's constructor then normalises
the quaternion of that R, which is what makes it a rotation again); the stereo edge's 1/p_z rounded to
float32 (the reference's cam_project works in float there); Huber's delta as the float32 of
sqrt(5.991) / sqrt(7.815).

The Jacobian is NOT the analytic formula: it is the central difference of e(exp(xi) * T) at xi = 0
in 50-digit arithmetic (step 1e-15: truncation ~ 1e-30 relative), with the unrounded 1/p_z.  The
analytic formula is what the kernel, the oracle and the restatement here use, so it is what is tested.

flawed(...) switches deliberate errors of the float64 restatement on, for the tests that show the
bounds discriminate.
"""
import contextlib
import math

import mpmath as mp
import numpy as np

import sim3_mp as sm
from sim3_mp import _f, _lin, _mm, _mv, _skew, group_errors, threshold_margin, within_bound  # noqa: F401

mp.mp.dps = 50
EPS = sm.EPS
DELTA = mp.mpf(10) ** -15
U52 = 2.0 ** -52
HUBER = {False: float(np.float32(math.sqrt(5.991))), True: float(np.float32(math.sqrt(7.815)))}   # [stereo]

FLAWS = ("J_rot_col_sign", "bf_row3_missing", "huber_weight_squared", "exp_eps_1e-4", "V_theta2")
_flaws = set()


@contextlib.contextmanager
def flawed(*names):
    assert all(n in FLAWS for n in names)
    _flaws.update(names)
    try:
        yield
    finally:
        _flaws.difference_update(names)


# ---------------------------------------------------------------- SE3 at 50 digits
def exp(u):
    """SE3Quat::exp of (omega, upsilon) -> (R, t)"""
    u = [_f(x) for x in u]
    w, ups = u[:3], u[3:6]
    theta = mp.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    Om = _skew(w)
    Om2 = _mm(Om, Om)
    if theta < EPS:
        V = _lin(1, Om, 1, Om2, 1)
        # SE3Quat(Quaterniond(R), t) normalises the quaternion of this R, which is no rotation
        q = sm.quat_from_R(V)[0]
        n = mp.sqrt(sum(v * v for v in q))
        R = sm.from_row([v / n for v in q] + [0, 0, 0, 1])[0]
    else:
        t2 = theta * theta
        R = _lin(mp.sin(theta) / theta, Om, (1 - mp.cos(theta)) / t2, Om2, 1)
        V = _lin((1 - mp.cos(theta)) / t2, Om, (theta - mp.sin(theta)) / (t2 * theta), Om2, 1)
    return R, _mv(V, ups)


def mul(a, b):
    return _mm(a[0], b[0]), [x + y for x, y in zip(_mv(a[0], b[1]), a[1])]


def smap(a, X):
    return [x + y for x, y in zip(_mv(a[0], [_f(v) for v in X]), a[1])]


def from_row(row):
    R, t, _ = sm.from_row(list(row[:7]) + [1.0])
    return R, t


def to_row(S):
    """7 mpf: the quaternion of R (Eigen's arms) with w >= 0, t"""
    q = sm.quat_from_R(S[0])[0]
    if q[3] < 0:
        q = [-v for v in q]
    return q + list(S[1])


def from_Tcw(T):
    """Converter::toSE3Quat of a float 4 x 4: the quaternion of its R (whatever R is), normalised
    to unit length with w >= 0 (SE3Quat's constructor), and its t -> (row of 7 mpf, arm)"""
    T = np.asarray(T, np.float32).reshape(4, 4)
    R = [[_f(T[i, j]) for j in range(3)] for i in range(3)]
    q, arm = sm.quat_from_R(R)
    n = mp.sqrt(sum(v * v for v in q))
    q = [v / n for v in q]
    if q[3] < 0:
        q = [-v for v in q]
    return q + [_f(T[i, 3]) for i in range(3)], arm


def to_Tcw(row):
    """SE3Quat -> the 16 entries of the float pose before their rounding to float32 (mpf)"""
    R, t = from_row(row)
    out = []
    for i in range(3):
        out += list(R[i]) + [t[i]]
    return out + [mp.mpf(0), mp.mpf(0), mp.mpf(0), mp.mpf(1)]


def rows8(rows):
    """rows of 7 (array or lists of mpf) with a unit scale appended: sim3_mp.group_errors's 'sim3' kind"""
    if isinstance(rows, np.ndarray):
        return np.concatenate([rows, np.ones((len(rows), 1))], 1)
    return [list(r) + [mp.mpf(1)] for r in rows]


def se3_errors(out, ref):
    """sim3_mp's measures of q (up to sign) and t (scaled by max(1, |t_ref|_inf)) for rows of 7"""
    E = group_errors("sim3", rows8(np.asarray(out, np.float64)), rows8(ref))
    del E["s"]
    return E


# ---------------------------------------------------------------- the edges at 50 digits
def round_f32(x):
    """the float32 nearest to the mpf x (normal range), as an mpf"""
    with mp.workprec(24):
        y = +x
    return y


def f32_midpoint_margin(x):
    """relative distance of the mpf x to the nearest midpoint between two neighbouring float32"""
    m, e = mp.frexp(abs(x))                 # x = m 2^e, 0.5 <= m < 1
    ulp = mp.ldexp(mp.mpf(1), e - 24)
    k = mp.floor(abs(x) / ulp)
    return abs(abs(x) - (k + mp.mpf(1) / 2) * ulp) / abs(x)


class Edge:
    """one observation: X (3 floats), obs (3 floats; obs[2] < 0: monocular), info, robust"""

    def __init__(self, X, obs, info, robust):
        self.X = [float(v) for v in X]
        self.obs = [float(v) for v in obs]
        self.info = float(info)
        self.robust = bool(robust)
        self.stereo = not (self.obs[2] < 0)
        self.delta = HUBER[self.stereo]


def error(T, e, cam, exact_invz=False):
    """the edge's error at T (R, t) -> (list of 2 or 3 mpf, p)"""
    fx, fy, cx, cy, bf = (_f(v) for v in cam)
    p = smap(T, e.X)
    if not e.stereo:
        return [_f(e.obs[0]) - (fx * p[0] / p[2] + cx), _f(e.obs[1]) - (fy * p[1] / p[2] + cy)], p
    invz = 1 / p[2]
    if not exact_invz:
        invz = round_f32(invz)
    u = p[0] * invz * fx + cx
    v = p[1] * invz * fy + cy
    return [_f(e.obs[0]) - u, _f(e.obs[1]) - v, _f(e.obs[2]) - (u - bf * invz)], p


def huber(e, chi2):
    """-> (rho0, weight): RobustKernelHuber on chi2, identity when the edge has no robust kernel"""
    d = _f(e.delta)
    if not e.robust or chi2 <= d * d:
        return chi2, mp.mpf(1)
    s = mp.sqrt(chi2)
    return 2 * s * d - d * d, d / s


def jacobian(T, e, cam):
    """3 x 6 (row 3 zero on a monocular edge): central differences of e(exp(xi) * T) at 50 digits,
    unrounded 1/p_z"""
    J = [[mp.mpf(0)] * 6 for _ in range(3)]
    for d in range(6):
        ev = []
        for sgn in (1, -1):
            xi = [mp.mpf(0)] * 6
            xi[d] = sgn * DELTA
            ev.append(error(mul(exp(xi), T), e, cam, exact_invz=True)[0])
        for k, (a, b) in enumerate(zip(*ev)):
            J[k][d] = (a - b) / (2 * DELTA)
    return J


def terms28(e, err, J, rho0, w):
    """rho0 | upper triangle of J^T (w info) J by rows | -J^T (w info) e"""
    W = w * _f(e.info)
    D = len(err)
    out = [rho0]
    for r in range(6):
        for c in range(r, 6):
            out.append(sum(J[k][r] * W * J[k][c] for k in range(D)))
    for r in range(6):
        out.append(-sum(J[k][r] * W * err[k] for k in range(D)))
    return out


def edge_reference(T_row, e, cam, with_J=True):
    """every per-edge quantity at the pose row T_row (7 float64) -> dict of mpf"""
    T = from_row(T_row)
    err, p = error(T, e, cam)
    chi2 = _f(e.info) * sum(v * v for v in err)
    rho0, w = huber(e, chi2)
    o = dict(err=err + [mp.mpf(0)] * (3 - len(err)), chi2=chi2, rho=rho0, w=w, pz=p[2],
             delta_margin=threshold_margin(chi2, _f(e.delta) ** 2))
    if e.stereo:
        o["invz_margin"] = f32_midpoint_margin(1 / p[2])
    if with_J:
        J = jacobian(T, e, cam)
        o["J"] = [v for row in J for v in row]
        o["terms"] = terms28(e, err, J, rho0, w)
    return o


# ---------------------------------------------------------------- the float64 restatement
def _skew64(w):
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], np.float64)


def _R64(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], np.float64)


def _row64(R, t):
    q = np.array(sm.quat_from_R(R.tolist(), math.sqrt)[0], np.float64)
    if q[3] < 0:
        q = -q
    return np.concatenate([q, t])


def exp64(u):
    """(R, t) float64"""
    u = np.asarray(u, np.float64)
    w, ups = u[:3], u[3:]
    theta = math.sqrt(w @ w)
    Om = _skew64(w)
    Om2 = Om @ Om
    if theta < (1e-4 if "exp_eps_1e-4" in _flaws else 0.00001):
        V = np.eye(3) + Om + Om2
        q = np.array(sm.quat_from_R(V.tolist(), math.sqrt)[0])
        R = _R64(q / math.sqrt(q @ q))       # SE3Quat's constructor normalises the quaternion
    else:
        t2 = theta * theta
        R = np.eye(3) + math.sin(theta) / theta * Om + (1 - math.cos(theta)) / t2 * Om2
        c = (theta - math.sin(theta)) / (t2 if "V_theta2" in _flaws else t2 * theta)
        V = np.eye(3) + (1 - math.cos(theta)) / t2 * Om + c * Om2
    return R, V @ ups


def f64(op, a, b=None):
    """the restatement on ABI rows, op by op like orbgpu_unit_se3"""
    out = []
    for i in range(len(a)):
        if op == "exp":
            out.append(_row64(*exp64(a[i])))
        elif op == "mul":
            Ra, Rb = _R64(a[i][:4]), _R64(b[i][:4])
            out.append(_row64(Ra @ Rb, Ra @ b[i][4:7] + a[i][4:7]))
        elif op == "map":
            out.append(_R64(a[i][:4]) @ np.asarray(b[i], np.float64) + a[i][4:7])
        elif op == "from_Tcw":
            T = np.asarray(a[i], np.float32).reshape(4, 4).astype(np.float64)
            q = np.array(sm.quat_from_R(T[:3, :3].tolist(), math.sqrt)[0])
            q = q / math.sqrt(q @ q)
            out.append(np.concatenate([-q if q[3] < 0 else q, T[:3, 3]]))
        else:
            assert op == "to_Tcw"
            T = np.eye(4)
            T[:3, :3], T[:3, 3] = _R64(a[i][:4]), a[i][4:7]
            out.append(T.astype(np.float32).reshape(16))
    return np.array(out)


def trial64(x, T_row):
    """exp(x) * T as a row of 7"""
    R, t = exp64(x)
    R0 = _R64(T_row[:4])
    return _row64(R @ R0, R @ np.asarray(T_row[4:7]) + t)


def edge_f64(T_row, e, cam):
    """err (3), chi2, rho, w, J (18, the chain rule d e / d p * [-[p]x | I]), terms (28) in float64"""
    fx, fy, cx, cy, bf = (float(v) for v in cam)
    p = _R64(T_row[:4]) @ np.array(e.X) + np.asarray(T_row[4:7], np.float64)
    x, y, z = p
    iz = 1.0 / z
    if e.stereo:
        izf = float(np.float32(iz))
        u, v = x * izf * fx + cx, y * izf * fy + cy
        err = np.array([e.obs[0] - u, e.obs[1] - v, e.obs[2] - (u - bf * izf)])
    else:
        err = np.array([e.obs[0] - (fx * x / z + cx), e.obs[1] - (fy * y / z + cy), 0.0])
    chi2 = e.info * float(err @ err)
    d = e.delta
    if e.robust and chi2 > d * d:
        s = math.sqrt(chi2)
        rho, w = 2 * s * d - d * d, d / s
        if "huber_weight_squared" in _flaws:
            w = w * w
    else:
        rho, w = chi2, 1.0
    # e = obs - proj(p): d e / d p = -d proj / d p; p(xi) = exp(xi) p: d p / d xi = [-[p]x | I]
    dproj = np.array([[fx * iz, 0, -fx * x * iz * iz], [0, fy * iz, -fy * y * iz * iz], [0, 0, 0]])
    if e.stereo:
        dproj[2] = dproj[0]
        if "bf_row3_missing" not in _flaws:
            dproj[2, 2] += bf * iz * iz      # u_r = u - bf / z
    J = -dproj @ np.concatenate([-_skew64(p), np.eye(3)], 1)
    if "J_rot_col_sign" in _flaws:
        J[:, 1] = -J[:, 1]
    W = w * e.info
    H = J.T @ (W * J)
    terms = np.concatenate([[rho], H[np.triu_indices(6)], -(J.T @ (W * err))])
    return dict(err=err, chi2=chi2, rho=rho, w=w, J=J.reshape(18), terms=terms)


def chi2_in_kernel_order(err, info, stereo):
    """chi2 of n edges in float64 in the kernel's operation order (pose_chi2): err n x 3, info n, stereo n"""
    err, info = np.asarray(err, np.float64).reshape(-1, 3), np.asarray(info, np.float64).reshape(-1)
    s = err[:, 0] * (info * err[:, 0])
    s = s + err[:, 1] * (info * err[:, 1])
    return np.where(np.asarray(stereo, bool).reshape(-1), s + err[:, 2] * (info * err[:, 2]), s)


def terms_in_kernel_order(J, err, chi2, info, delta, robust):
    """The 28 terms of n edges in float64 in the operation order of the kernel's per-edge body
    (pose_sys_terms, csrc/pose_opt.hip) from given J (n x 18), err (n x 3), chi2, info, Huber delta
    and robust flag (n each): what the device's terms are held to bit for bit.  test_pose_mp_cpu.py
    holds this restatement to the 50-digit terms."""
    J, err = np.asarray(J, np.float64).reshape(-1, 18), np.asarray(err, np.float64).reshape(-1, 3)
    c, info, d = (np.asarray(v, np.float64).reshape(-1) for v in (chi2, info, delta))
    rb = np.asarray(robust, bool).reshape(-1)
    dsqr = d * d
    out = np.zeros((len(J), 28))
    with np.errstate(invalid="ignore", divide="ignore"):
        sq = np.sqrt(c)
        inside = ~rb | (c <= dsqr)
        out[:, 0] = np.where(inside, c, (2 * sq) * d - dsqr)
        r1 = np.where(rb & ~(c <= dsqr), d / sq, 1.0)
        wgt = np.where(rb, r1 * info, info)
        omr = -(info[:, None] * err)
        omr = np.where(rb[:, None], omr * r1[:, None], omr)
        q = 1
        for r in range(6):
            sb = np.zeros(len(J))
            for k in range(3):
                sb = sb + J[:, k * 6 + r] * omr[:, k]
            out[:, 22 + r] = sb
            for cc in range(r, 6):
                hh = np.zeros(len(J))
                for k in range(3):
                    hh = hh + (J[:, k * 6 + r] * wgt) * J[:, k * 6 + cc]
                out[:, q] = hh
                q += 1
    return out


# ---------------------------------------------------------------- error measures of the edges
def _scaled_max(vals, ref):
    ref = list(ref)
    return float(max(abs(_f(a) - b) for a, b in zip(vals, ref)) / max(1, max(abs(b) for b in ref)))


def edge_errors(outs, refs, keys=("err", "chi2", "rho", "J", "terms")):
    """Largest distance to the 50-digit values over the edges, per quantity: vectors scaled by
    max(1, |ref|_inf) of the edge's vector, scalars by max(1, |ref|).  outs / refs: lists of dicts."""
    E = {}
    for o, r in zip(outs, refs):
        for k in keys:
            if k not in r or k not in o:
                continue
            v = _scaled_max(np.atleast_1d(o[k]), r[k] if isinstance(r[k], list) else [r[k]])
            E[k] = max(E.get(k, 0.0), v)
    return E
