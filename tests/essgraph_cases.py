"""Pose graphs for Optimizer::OptimizeEssentialGraph and its NumPy float64 reference.

The CPU oracle (oracle/ba.c) has no essential-graph path, so the parity reference of this call
is the restatement below of g2o's sim3.h / EdgeSim3 / OptimizationAlgorithmLevenberg as
ORB-SLAM2 drives them (Optimizer.cc:781-1044): Sim3 exp / log on rotation matrices, numeric
central-difference Jacobians (delta 1e-9), dense H, the LM control of oracle/ba.c.  Everything is
batched over edges.

Because of the 1e-9 numeric Jacobians the reference is only defined to about 1e-5 in pose after
an LM step that leaves a residual: `variant` selects evaluations that differ only in rounding
(edge order, LU versus Cholesky, association of the error product) so that tests can measure that
spread and bound the GPU against it.
"""
import functools

import numpy as np

DELTA = 1e-9
EPS = 0.00001


# ---------------------------------------------------------------- Sim3 on (R, t, s), batched
def skew(w):
    O = np.zeros(w.shape[:-1] + (3, 3))
    O[..., 0, 1], O[..., 0, 2] = -w[..., 2], w[..., 1]
    O[..., 1, 0], O[..., 1, 2] = w[..., 2], -w[..., 0]
    O[..., 2, 0], O[..., 2, 1] = -w[..., 1], w[..., 0]
    return O


def _abc(theta, sigma, s):
    """A, B, C of g2o::Sim3's exp and log (sim3.h:64-146): four branches on theta, sigma."""
    smallT, smallS = theta < EPS, np.abs(sigma) < EPS
    th = np.where(smallT, 1.0, theta)
    sg = np.where(smallS, 1.0, sigma)
    th2, sg2 = th * th, sg * sg
    sn, cs = np.sin(th), np.cos(th)
    C = np.where(smallS, 1.0, (s - 1) / sg)
    a, b, c = s * sn, s * cs, th2 + sg2
    A = np.where(smallT, np.where(smallS, 0.5, ((sg - 1) * s + 1) / sg2),
                 np.where(smallS, (1 - cs) / th2, (a * sg + (1 - b) * th) / (th * c)))
    B = np.where(smallT, np.where(smallS, 1. / 6., ((0.5 * sg2 - sg + 1) * s) / (sg2 * sg)),   # g2o's B, as it stands
                 np.where(smallS, (th - sn) / (th2 * th), (C - ((b - 1) * sg + a * th) / c) / th2))
    return A, B, C


def s3_exp(u):
    u = np.asarray(u, np.float64)
    w, ups, sigma = u[..., :3], u[..., 3:6], u[..., 6]
    theta = np.sqrt((w * w).sum(-1))
    s = np.exp(sigma)
    Om = skew(w)
    Om2 = Om @ Om
    A, B, C = _abc(theta, sigma, s)
    I = np.eye(3)
    small = theta < EPS
    th = np.where(small, 1.0, theta)
    ra = np.where(small, 1.0, np.sin(th) / th)
    rb = np.where(small, 1.0, (1 - np.cos(th)) / (th * th))
    R = I + ra[..., None, None] * Om + rb[..., None, None] * Om2
    W = A[..., None, None] * Om + B[..., None, None] * Om2 + C[..., None, None] * I
    return R, (W @ ups[..., None])[..., 0], s


def s3_log(S):
    R, t, s = S
    sigma = np.log(s)
    d = 0.5 * (np.trace(R, axis1=-2, axis2=-1) - 1)
    dR = np.stack([R[..., 2, 1] - R[..., 1, 2], R[..., 0, 2] - R[..., 2, 0], R[..., 1, 0] - R[..., 0, 1]], -1)
    near = d > 1 - EPS
    dd = np.where(near, 0.0, np.clip(d, -1.0, 1.0))
    theta = np.where(near, 0.0, np.arccos(dd))
    k = np.where(near, 0.5, theta / (2 * np.sqrt(1 - dd * dd)))
    w = k[..., None] * dR
    A, B, C = _abc(theta, sigma, s)   # theta = 0 selects the near-identity branches
    Om = skew(w)
    W = A[..., None, None] * Om + B[..., None, None] * (Om @ Om) + C[..., None, None] * np.eye(3)
    ups = np.linalg.solve(W, t[..., None])[..., 0]
    return np.concatenate([w, ups, sigma[..., None]], -1)


def mul(a, b):
    Ra, ta, sa = a
    Rb, tb, sb = b
    return Ra @ Rb, sa[..., None] * (Ra @ tb[..., None])[..., 0] + ta, sa * sb


def inv(a):
    R, t, s = a
    Rt = np.swapaxes(R, -1, -2)
    return Rt, (-1.0 / s)[..., None] * (Rt @ t[..., None])[..., 0], 1.0 / s


def smap(a, X):
    R, t, s = a
    return s[..., None] * (R @ X[..., None])[..., 0] + t


def take(S, idx):
    return S[0][idx], S[1][idx], S[2][idx]


def quat_to_R(q):
    q = np.asarray(q, np.float64)
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    R = np.empty(q.shape[:-1] + (3, 3))
    R[..., 0, 0] = 1 - 2 * (y * y + z * z)
    R[..., 0, 1] = 2 * (x * y - z * w)
    R[..., 0, 2] = 2 * (x * z + y * w)
    R[..., 1, 0] = 2 * (x * y + z * w)
    R[..., 1, 1] = 1 - 2 * (x * x + z * z)
    R[..., 1, 2] = 2 * (y * z - x * w)
    R[..., 2, 0] = 2 * (x * z - y * w)
    R[..., 2, 1] = 2 * (y * z + x * w)
    R[..., 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def R_to_quat(R):
    """Unit quaternion (x, y, z, w), w >= 0, of one rotation matrix (Shepperd)."""
    R = np.asarray(R, np.float64)
    K = np.array([R[0, 0] + R[1, 1] + R[2, 2], R[0, 0], R[1, 1], R[2, 2]])
    i = int(np.argmax(K))
    if i == 0:
        w = 0.5 * np.sqrt(1 + K[0])
        q = np.array([(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w])
    else:
        a = i - 1
        b, c = (a + 1) % 3, (a + 2) % 3
        x = 0.5 * np.sqrt(1 + R[a, a] - R[b, b] - R[c, c])
        q = np.zeros(4)
        q[a] = x
        q[b] = (R[b, a] + R[a, b]) / (4 * x)
        q[c] = (R[c, a] + R[a, c]) / (4 * x)
        q[3] = (R[c, b] - R[b, c]) / (4 * x)
    q /= np.linalg.norm(q)
    return q if q[3] >= 0 else -q


def rows_to_sim3(rows):
    rows = np.asarray(rows, np.float64)
    return quat_to_R(rows[..., :4]), rows[..., 4:7].copy(), rows[..., 7].copy()


def sim3_to_rows(S):
    R, t, s = S
    out = np.zeros((len(s), 8))
    for v in range(len(s)):
        out[v, :4] = R_to_quat(R[v])
        out[v, 4:7] = t[v]
        out[v, 7] = s[v]
    return out


def pose_distance(rows_a, rows_b):
    """max over vertices of |log(S_a * S_b^-1)|_inf"""
    return float(np.abs(s3_log(mul(rows_to_sim3(rows_a), inv(rows_to_sim3(rows_b))))).max())


# ---------------------------------------------------------------- Sim3 on (q, t, s), batched
# The same group with the rotation kept as a quaternion (x, y, z, w), as g2o::Sim3 stores it:
# another evaluation of the reference that differs only in rounding.
def qmul(a, b):
    ax, ay, az, aw = (a[..., i] for i in range(4))
    bx, by, bz, bw = (b[..., i] for i in range(4))
    return np.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz], -1)


def qrot(q, v):
    uv = 2 * np.cross(q[..., :3], v)
    return v + q[..., 3:4] * uv + np.cross(q[..., :3], uv)


class MatrixAlgebra:
    """Sim3 as (R, t, s): the functions above"""
    mul, inv, exp, log = staticmethod(mul), staticmethod(inv), staticmethod(s3_exp), staticmethod(s3_log)
    from_rows, to_rows = staticmethod(rows_to_sim3), staticmethod(sim3_to_rows)


class QuatAlgebra:
    """Sim3 as (q, t, s); exp and log go through the rotation matrix as g2o's do"""
    @staticmethod
    def mul(a, b):
        return qmul(a[0], b[0]), a[2][..., None] * qrot(a[0], b[1]) + a[1], a[2] * b[2]

    @staticmethod
    def inv(a):
        qc = a[0] * np.array([-1.0, -1.0, -1.0, 1.0])
        return qc, qrot(qc, (-1.0 / a[2])[..., None] * a[1]), 1.0 / a[2]

    @staticmethod
    def exp(u):
        R, t, s = s3_exp(u)
        q = np.stack([R_to_quat(r) for r in R.reshape(-1, 3, 3)]).reshape(R.shape[:-2] + (4,))
        return q, t, s

    @staticmethod
    def log(S):
        return s3_log((quat_to_R(S[0]), S[1], S[2]))

    @staticmethod
    def from_rows(rows):
        rows = np.asarray(rows, np.float64)
        return rows[..., :4].copy(), rows[..., 4:7].copy(), rows[..., 7].copy()

    @staticmethod
    def to_rows(S):
        return np.concatenate([S[0], S[1], S[2][..., None]], -1)


# ---------------------------------------------------------------- the reference optimiser
def measurements(problem, A=MatrixAlgebra):
    Scw, Snc = A.from_rows(problem["Scw"]), A.from_rows(problem["ScwNonCorrected"])
    ei, ej, loop = problem["edge_i"], problem["edge_j"], problem["edge_loop"].astype(bool)
    Ml = A.mul(take(Scw, ej), A.inv(take(Scw, ei)))
    Mn = A.mul(take(Snc, ej), A.inv(take(Snc, ei)))
    return tuple(np.where(loop.reshape((-1,) + (1,) * (l.ndim - 1)), l, m) for l, m in zip(Ml, Mn))


def edge_errors(M, Si, Sj, assoc, A=MatrixAlgebra):
    if assoc == 0:
        return A.log(A.mul(A.mul(M, Si), A.inv(Sj)))
    return A.log(A.mul(M, A.mul(Si, A.inv(Sj))))


def numeric_jacobian(M, est, ei, ej, fix, assoc=0, A=MatrixAlgebra):
    """g2o's central differences (delta 1e-9) of every edge by both of its vertices, fixed ones
    included: J[side, e, k, d]"""
    J = np.zeros((2, len(ei), 7, 7))
    for side, idx in ((0, ei), (1, ej)):
        for d in range(7):
            ev = []
            for sgn in (1.0, -1.0):
                add = np.zeros(7)
                add[d] = sgn * DELTA
                if fix:
                    add[6] = 0
                P = A.mul(A.exp(add), take(est, idx))
                Si, Sj = (P, take(est, ej)) if side == 0 else (take(est, ei), P)
                ev.append(edge_errors(M, Si, Sj, assoc, A))
            J[side, :, :, d] = (ev[0] - ev[1]) / (2 * DELTA)
    return J


VARIANTS = ("natural_cholesky", "reversed_lu", "assoc", "quaternion")


def ref_optimize(problem, nIterations=20, variant=0):
    """-> dict(Scw rows, chi2 trace, n_solves, lm_trials).  variant 0: edges in order, Cholesky,
    (M Si) Sj^-1; 1: edges summed in reverse order, LU; 2: M (Si Sj^-1); 3: as 0 with the rotations
    kept as quaternions (QuatAlgebra)."""
    assoc = 1 if variant == 2 else 0
    A = QuatAlgebra if variant == 3 else MatrixAlgebra
    est = A.from_rows(problem["Scw"])
    nKF = len(est[2])
    ei, ej = np.asarray(problem["edge_i"]), np.asarray(problem["edge_j"])
    nE = len(ei)
    fixed = np.asarray(problem["fixed"]).astype(bool)
    fix = bool(problem["bFixScale"])
    has = np.zeros(nKF, bool)
    has[ei] = True
    has[ej] = True
    sys_idx = -np.ones(nKF, int)
    free = np.flatnonzero(~fixed & has)
    sys_idx[free] = np.arange(len(free))
    n = 7 * len(free)
    M = measurements(problem, A) if nE else None

    def errors(e):
        return edge_errors(M, take(e, ei), take(e, ej), assoc, A)

    def chi2_of(err):
        return float((err * err).sum())

    trace = [chi2_of(errors(est)) if nE else 0.0]
    out = dict(n_solves=0, lm_trials=0, trials_per_solve=[], trial_chi2=[])
    if nIterations > 0 and nE and n:
        lam, ni, nBad = 1e-16, 2.0, 0
        order = range(nE - 1, -1, -1) if variant == 1 else range(nE)
        for _ in range(nIterations):
            err = errors(est)
            J = numeric_jacobian(M, est, ei, ej, fix, assoc, A)
            H, b = np.zeros((n, n)), np.zeros(n)
            for e in order:
                a, c = sys_idx[ei[e]], sys_idx[ej[e]]
                Ji, Jj = J[0, e], J[1, e]
                if a >= 0:
                    H[7 * a:7 * a + 7, 7 * a:7 * a + 7] += Ji.T @ Ji
                    b[7 * a:7 * a + 7] -= Ji.T @ err[e]
                if c >= 0:
                    H[7 * c:7 * c + 7, 7 * c:7 * c + 7] += Jj.T @ Jj
                    b[7 * c:7 * c + 7] -= Jj.T @ err[e]
                if a >= 0 and c >= 0:
                    H[7 * a:7 * a + 7, 7 * c:7 * c + 7] += Ji.T @ Jj
                    H[7 * c:7 * c + 7, 7 * a:7 * a + 7] += Jj.T @ Ji
            currentChi = iniChi = chi2_of(err)
            qmax, rho = 0, 0.0
            x = np.zeros(n)
            while True:
                Hl = H + lam * np.eye(n)
                ok = True
                try:
                    if variant == 1:
                        x = np.linalg.solve(Hl, b)
                    else:
                        L = np.linalg.cholesky(Hl)
                        x = np.linalg.solve(L.T, np.linalg.solve(L, b))
                except np.linalg.LinAlgError:
                    ok = False
                if fix:
                    x[6::7] = 0
                bak = est
                U = A.exp(x.reshape(-1, 7))
                new = A.mul(U, take(est, free))
                est = tuple(a.copy() for a in est)
                est[0][free], est[1][free], est[2][free] = new
                tempChi = chi2_of(errors(est))
                if not ok or not np.isfinite(tempChi):
                    tempChi = np.finfo(np.float64).max
                scale = float(x @ (lam * x + b)) + 1e-3
                rho = (currentChi - tempChi) / scale
                if rho > 0 and np.isfinite(tempChi):
                    alpha = min(1. - (2 * rho - 1) ** 3, 2. / 3.)
                    lam *= max(1. / 3., alpha)
                    ni = 2.0
                    currentChi = tempChi
                else:
                    lam *= ni
                    ni *= 2
                    est = bak
                qmax += 1
                out["lm_trials"] += 1
                out["trial_chi2"].append(tempChi)
                if not (rho < 0 and qmax < 10):
                    break
            out["n_solves"] += 1
            out["trials_per_solve"].append(qmax)
            trace.append(currentChi)
            if qmax == 10 or rho == 0:
                break
            nBad = nBad + 1 if (iniChi - currentChi) * 1e3 < iniChi else 0
            if nBad >= 3:
                break
    out["Scw"] = A.to_rows(est)
    out["chi2"] = np.array(trace)
    return out


def ref_writeback(problem, Scw_out):
    """(Tcw float32 nKF x 4 x 4, mp_pos float32) from the corrected rows, in float64 then rounded."""
    R, t, s = rows_to_sim3(Scw_out)
    T = np.zeros((len(s), 4, 4))
    T[:, :3, :3] = R
    T[:, :3, 3] = t / s[:, None]
    T[:, 3, 3] = 1
    mp = np.asarray(problem.get("mp_pos", np.zeros((0, 3), np.float32)), np.float32)
    ref = np.asarray(problem.get("mp_ref", np.zeros(0, np.int32)))
    out = mp.copy()
    m = ref >= 0
    if m.any():
        S0 = rows_to_sim3(problem["Scw"])
        c = smap(take(S0, ref[m]), mp[m].astype(np.float64))
        out[m] = smap(inv(take((R, t, s), ref[m])), c).astype(np.float32)
    return T.astype(np.float32), out


# ---------------------------------------------------------------- graphs
def _truth(N):
    """Cameras on a radius-10 circle that stops one step short of closing: Tcw as Sim3, scale 1."""
    a = 2 * np.pi * np.arange(N) / N
    Rwc = np.zeros((N, 3, 3))
    Rwc[:, 0, 0], Rwc[:, 0, 1], Rwc[:, 1, 0], Rwc[:, 1, 1], Rwc[:, 2, 2] = np.cos(a), -np.sin(a), np.sin(a), np.cos(a), 1
    c = np.stack([10 * np.cos(a), 10 * np.sin(a), 0.3 * np.sin(3 * a)], -1)
    Rcw = np.swapaxes(Rwc, -1, -2)
    return Rcw, -(Rcw @ c[..., None])[..., 0], np.ones(N)


def _one(S, k):
    return S[0][k], S[1][k], S[2][k]


def _stack(lst):
    return np.stack([x[0] for x in lst]), np.stack([x[1] for x in lst]), np.array([x[2] for x in lst])


def _topology(N, n_corrected):
    corrected = list(range(N - n_corrected, N))
    loop_pairs = [(c, j) for c in corrected for j in (0, 1)]
    joined = {frozenset(p) for p in loop_pairs}
    normal = [(i, i - k) for i in range(1, N) for k in (1, 2, 3) if i - k >= 0 and frozenset((i, i - k)) not in joined]
    return corrected, loop_pairs, normal


def _pack(N, Scw, Snc, loop_pairs, normal, fix_scale, loop_flag=True):
    edges = loop_pairs + normal
    fixed = np.zeros(N, np.uint8)
    fixed[0] = 1
    return dict(Scw=sim3_to_rows(Scw), ScwNonCorrected=sim3_to_rows(Snc), fixed=fixed,
                edge_i=np.array([e[0] for e in edges], np.int32), edge_j=np.array([e[1] for e in edges], np.int32),
                edge_loop=np.array([1 if loop_flag else 0] * len(loop_pairs) + [0] * len(normal), np.uint8),
                bFixScale=int(fix_scale))


def ring_graph(N, seed, scale_drift=0.0, rot_sigma=0.03, trans_sigma=0.1, scale_sigma=0.0, n_corrected=4,
               fix_scale=True):
    """Keyframe 0 is the fixed loop keyframe; odometry drift composed on the left per step; the last
    n_corrected keyframes carry corrected estimates that put the last keyframe where the loop
    says it is (CorrectedSim3 = Sic * corrected Scw, LoopClosing.cc:424-440), their drifted Sim3
    in ScwNonCorrected; loop edges from each corrected keyframe to keyframes 0 and 1; normal edges
    i -> i-1, i-2, i-3 except pairs a loop edge joins."""
    rng = np.random.default_rng(seed)
    T = _truth(N)
    S = [_one(T, 0)]
    for k in range(1, N):
        rel = mul(_one(T, k), inv(_one(T, k - 1)))
        u = np.concatenate([rot_sigma * rng.standard_normal(3), trans_sigma * rng.standard_normal(3),
                            [0.0 if fix_scale else scale_drift + scale_sigma * rng.standard_normal()]])
        S.append(mul(s3_exp(u), mul(rel, S[-1])))
    corrected, loop_pairs, normal = _topology(N, n_corrected)
    Scw = list(S)
    last_corr = _one(T, N - 1)
    for c in corrected:
        Scw[c] = mul(mul(S[c], inv(S[N - 1])), last_corr)
    return _pack(N, _stack(Scw), _stack(S), loop_pairs, normal, fix_scale)


def zero_residual_graph(N, seed, fix_scale=True, n_corrected=4, sigma=(0.03, 0.2, 0.05)):
    """The ring's topology with every measurement taken from one ground truth (per-keyframe scales
    when the scale is free) and the estimates perturbed.  The call takes its measurements from the
    Sim3 tables, so the truth sits in ScwNonCorrected, every edge is a normal edge and Scw holds
    the perturbed estimates.  -> (problem, truth rows)"""
    rng = np.random.default_rng(seed)
    R, t, s = _truth(N)
    if not fix_scale:
        s = np.exp(0.1 * rng.standard_normal(N))
        s[0] = 1.0
    G = (R, t, s)
    u = np.concatenate([sigma[0] * rng.standard_normal((N, 3)), sigma[1] * rng.standard_normal((N, 3)),
                        (0.0 if fix_scale else sigma[2]) * rng.standard_normal((N, 1))], -1)
    u[0] = 0
    est = mul(s3_exp(u), G)
    _, loop_pairs, normal = _topology(N, n_corrected)
    pr = _pack(N, est, G, loop_pairs, normal, fix_scale, loop_flag=False)
    return pr, pr["ScwNonCorrected"].copy()


# Seeds of the zero-residual cases.  With the scale free, whether g2o's optimiser reaches the truth
# is decided by rounding: an update whose rotation is below 1e-5 while its scale step is not takes
# the theta ~ 0, sigma != 0 branch of Sim3's exp, whose B (about 1 / sigma^3, as g2o writes it)
# multiplies Omega^2 into a wrong translation; the trial is rejected ten times and the optimiser
# stops a few 1e-3 from the truth.  Of seeds 1..8 the three reference variants all reach the truth
# for 4 (N = 12), 4 (N = 40) and 3 (N = 160) seeds, all stall for 2, 2 and 1, and disagree on the
# rest.  The tests use seeds on which all three agree with a margin (test_essgraph_cpu.py asserts
# it); scale-fixed graphs have sigma = 0 and never meet the branch.
ZERO_SEEDS = {(12, True): 1, (12, False): 1, (40, True): 1, (40, False): 5, (160, True): 1, (160, False): 2}


def zero_residual_case(N, fix_scale):
    return zero_residual_graph(N, seed=ZERO_SEEDS[(N, bool(fix_scale))], fix_scale=fix_scale)


# the ring cases of the parity tests: (N, drift (rot, trans, scale) sigma, scale fixed)
RING_CASES = {
    "n12_fix": dict(N=12, seed=3, rot_sigma=0.03, trans_sigma=0.1, scale_sigma=0.05, fix_scale=True),
    "n12_free": dict(N=12, seed=3, rot_sigma=0.03, trans_sigma=0.1, scale_sigma=0.05, fix_scale=False),
    "n40_fix": dict(N=40, seed=5, rot_sigma=0.02, trans_sigma=0.1, scale_sigma=0.03, fix_scale=True),
    "n40_free": dict(N=40, seed=5, rot_sigma=0.02, trans_sigma=0.1, scale_sigma=0.03, fix_scale=False),
}


# A ring whose first Gauss-Newton step overshoots: with lambda0 = 1e-16 the first nine trials of
# iteration 0 are rejected (chi2 1.32e4 -> 1.48e4) and the tenth, at lambda = 2^45 * 1e-16 = 3.5e-3,
# is accepted (1.19e4); ten trials end the optimisation.  Every retry must be solved with the b of
# the linearisation point, not with the rejected trial's errors.
REJECT_CASE = dict(N=12, seed=2, rot_sigma=0.5, trans_sigma=2.0, scale_sigma=0.1, fix_scale=True)


@functools.lru_cache(maxsize=None)
def reject_case():
    """(problem, the four reference variants): computed once and shared (do not modify).  The step
    that is finally accepted runs along a weakly constrained direction, which amplifies the numeric
    Jacobians' rounding pattern: chi2 after it is 11851.763 / 11851.763 / 11851.877 with rotation
    matrices and 11853.246 with quaternions (1.3e-4 relative), while 1-ulp changes of the inputs
    move either by less than 1e-4.  The spread the GPU is held to therefore includes the
    quaternion variant, the arithmetic g2o itself uses."""
    pr = ring_graph(**REJECT_CASE)
    return pr, tuple(ref_optimize(pr, 20, v) for v in range(4))


# A ring with a large scale drift whose Gauss-Newton step overshoots by 35 to 65 % of chi2 at every
# lambda the ten trials reach (lambda <= 3.5e-3 cannot shorten it): ten rejections end the
# optimisation with the estimates restored.  Sharp: nothing here depends on the Jacobians' noise.
REJECT_ALL_CASE = dict(N=12, seed=1, scale_drift=-0.4, rot_sigma=0.3, trans_sigma=1.0, scale_sigma=0.3,
                       fix_scale=False)


@functools.lru_cache(maxsize=None)
def reject_all_case():
    pr = ring_graph(**REJECT_ALL_CASE)
    return pr, tuple(ref_optimize(pr, 20, v) for v in range(4))


@functools.lru_cache(maxsize=None)
def ring_case(name):
    return ring_graph(**RING_CASES[name])


@functools.lru_cache(maxsize=None)
def ring_reference(name, nIterations=20):
    """The three reference variants of a ring case, computed once and shared (do not modify)."""
    pr = ring_case(name)
    return tuple(ref_optimize(pr, nIterations, v) for v in range(3))


def variant_spread(refs):
    """(relative spread of the initial chi2, of the final chi2, largest pose distance between variants)"""
    c0 = np.array([r["chi2"][0] for r in refs])
    c1 = np.array([r["chi2"][-1] for r in refs])
    pose = max(pose_distance(refs[a]["Scw"], refs[b]["Scw"]) for a in range(len(refs)) for b in range(a))
    return (c0.max() - c0.min()) / c0.max(), (c1.max() - c1.min()) / c1.max(), pose


# ---------------------------------------------------------------- graphs of the stage tests
def flip_edges(pr, seed):
    """The same graph with the direction of a seeded half of the edges reversed.  The call derives
    each measurement Sji from the tables, so a reversed edge is as consistent as the original."""
    rng = np.random.default_rng(seed)
    nE = len(pr["edge_i"])
    swap = np.zeros(nE, bool)
    swap[rng.permutation(nE)[:nE // 2]] = True
    out = dict(pr)
    out["edge_i"] = np.where(swap, pr["edge_j"], pr["edge_i"]).astype(np.int32)
    out["edge_j"] = np.where(swap, pr["edge_i"], pr["edge_j"]).astype(np.int32)
    return out


def system_index(pr):
    """sysIdx (free vertices with an edge, in the caller's order; -1 otherwise) and their count"""
    nKF = len(pr["fixed"])
    has = np.zeros(nKF, bool)
    has[pr["edge_i"]] = True
    has[pr["edge_j"]] = True
    sys_idx = -np.ones(nKF, np.int32)
    free = np.flatnonzero(~np.asarray(pr["fixed"]).astype(bool) & has)
    sys_idx[free] = np.arange(len(free))
    return sys_idx, len(free)


def edge_orders(pr):
    """(edges with both ends in the system and sysIdx[i] < sysIdx[j], with sysIdx[i] > sysIdx[j])"""
    s, _ = system_index(pr)
    a, b = s[pr["edge_i"]], s[pr["edge_j"]]
    both = (a >= 0) & (b >= 0)
    return int((both & (a < b)).sum()), int((both & (a > b)).sum())


def _append_edges(pr, pairs):
    out = dict(pr)
    out["edge_i"] = np.concatenate([pr["edge_i"], [p[0] for p in pairs]]).astype(np.int32)
    out["edge_j"] = np.concatenate([pr["edge_j"], [p[1] for p in pairs]]).astype(np.int32)
    out["edge_loop"] = np.concatenate([pr["edge_loop"], np.zeros(len(pairs), np.uint8)])
    return out


def perturbed_graph(N, edges, fixed, seed, fix_scale):
    """Measurements from a ground truth on the circle (in ScwNonCorrected; every edge a normal edge),
    estimates perturbed by (0.02, 0.1, 0.02) in (rotation, translation, log scale): every edge has a
    residual of that size.  Vectorised: for graphs of a thousand keyframes."""
    rng = np.random.default_rng(seed)
    R, t, s = _truth(N)
    if not fix_scale:
        s = np.exp(0.05 * rng.standard_normal(N))
    G = (R, t, s)
    u = np.concatenate([0.02 * rng.standard_normal((N, 3)), 0.1 * rng.standard_normal((N, 3)),
                        (0.0 if fix_scale else 0.02) * rng.standard_normal((N, 1))], -1)
    fx = np.zeros(N, np.uint8)
    fx[list(fixed)] = 1
    return dict(Scw=sim3_to_rows(mul(s3_exp(u), G)), ScwNonCorrected=sim3_to_rows(G), fixed=fx,
                edge_i=np.array([e[0] for e in edges], np.int32), edge_j=np.array([e[1] for e in edges], np.int32),
                edge_loop=np.zeros(len(edges), np.uint8), bFixScale=int(fix_scale))


def _band(N):
    return [(i, i - k) for i in range(1, N) for k in (1, 2, 3) if i - k >= 0]


@functools.lru_cache(maxsize=None)
def stage_graph(name):
    """The graphs of test_gpu_essgraph_stages.py (do not modify); every one has edges in both
    directions of the system order.
      g1_free / g1_fix   the n12 rings, 77 rows
      ring20 / ring21    rings with 20 / 21 free vertices: 140 and 147 rows, the two sides of the
                         dense solver's limit of 144
      hub                80 keyframes (scale fixed), vertex 5 joined to every vertex the ring does not join it to,
                         five of those pairs twice: degree above 64, 553 rows
      split              two rings of 13 keyframes with a fixed vertex each and no edge between them,
                         one free vertex of the second joined to fixed vertices only, and between the
                         two an edge-less free vertex (a gap in sysIdx): 27 keyframes, 168 rows
      few_free           1,370 keyframes, five of them free, the band's edge list cut to 4,097
      e1 / e63 / e64     one free vertex and one edge; nine free (63 rows) and 63 edges; five and 64
      e65                a chain of 65 edges with 64 free vertices: 448 rows
      big                586 free vertices in a band: 4,102 rows"""
    if name in ("g1_free", "g1_fix"):
        return flip_edges(ring_case("n12_free" if name == "g1_free" else "n12_fix"), 11)
    if name in ("ring20", "ring21"):
        N = 21 if name == "ring20" else 22
        return flip_edges(ring_graph(N=N, seed=9, rot_sigma=0.03, trans_sigma=0.1, scale_sigma=0.04, fix_scale=False), 12)
    if name == "hub":
        # scale fixed: with it free the reference's own rounding variants end 3e-2 apart here (ten
        # rejected trials in the theta ~ 0, sigma != 0 arm of exp, see ZERO_SEEDS); fixed they agree to 4e-6
        pr = ring_graph(N=80, seed=4, rot_sigma=0.01, trans_sigma=0.05, scale_sigma=0.01, fix_scale=True)
        joined = {frozenset(p) for p in zip(pr["edge_i"].tolist(), pr["edge_j"].tolist())}
        spokes = [(v, 5) for v in range(80) if v != 5 and frozenset((v, 5)) not in joined]
        return flip_edges(_append_edges(pr, spokes + spokes[10:15]), 13)
    if name == "split":
        a = ring_graph(N=13, seed=21, rot_sigma=0.03, trans_sigma=0.1, scale_sigma=0.04, fix_scale=False)
        b = ring_graph(N=13, seed=22, rot_sigma=0.03, trans_sigma=0.1, scale_sigma=0.04, fix_scale=False)
        keep = (b["edge_i"] != 6) & (b["edge_j"] != 6)   # vertex 6 of the second ring keeps no edge to a free vertex
        lone = a["Scw"][4:5].copy()
        lone[0, 4:7] += 2.0
        pr = dict(Scw=np.concatenate([a["Scw"], lone, b["Scw"]]),
                  ScwNonCorrected=np.concatenate([a["ScwNonCorrected"], lone, b["ScwNonCorrected"]]),
                  fixed=np.concatenate([a["fixed"], [0], b["fixed"]]).astype(np.uint8),
                  edge_i=np.concatenate([a["edge_i"], b["edge_i"][keep] + 14]).astype(np.int32),
                  edge_j=np.concatenate([a["edge_j"], b["edge_j"][keep] + 14]).astype(np.int32),
                  edge_loop=np.concatenate([a["edge_loop"], b["edge_loop"][keep]]), bFixScale=0)
        Scw = pr["Scw"].copy()
        Scw[20, 4:7] += 0.05   # a residual on that vertex's edges (its tables agree otherwise)
        pr["Scw"] = Scw
        return flip_edges(_append_edges(pr, [(20, 14), (14, 20), (20, 0)]), 14)
    if name == "few_free":
        return flip_edges(perturbed_graph(1370, _band(1370)[:4097], set(range(1370)) - {40, 41, 42, 43, 900}, 31, False), 15)
    if name == "e1":
        return perturbed_graph(30, [(7, 6)], set(range(30)) - {7}, 32, False)
    if name == "e63":
        return flip_edges(perturbed_graph(30, _band(30)[:63], set(range(30)) - set(range(2, 11)), 33, False), 16)
    if name == "e64":
        return flip_edges(perturbed_graph(30, _band(30)[:64], set(range(30)) - {3, 4, 5, 6, 15}, 34, False), 17)
    if name == "e65":
        return flip_edges(perturbed_graph(66, [(i, i - 1) for i in range(1, 66)], {0, 1}, 35, False), 18)
    if name == "big":
        return flip_edges(perturbed_graph(587, _band(587), {0}, 36, False), 19)
    raise KeyError(name)


STAGE_GRAPHS = ("g1_free", "g1_fix", "ring20", "ring21", "hub", "split", "few_free", "e1", "e63", "e64", "e65", "big")


def gather_lists(ei, ej, sys_idx, nV, flip_side_when_a_below_b=False):
    """{(a, b), a <= b in system order: [(edge, side of a)] in edge order} from the edge list alone
    (the deliberate error: the side bit of the a < b entries flipped)"""
    lists = {}
    for e in range(len(ei)):
        a, b = int(sys_idx[ei[e]]), int(sys_idx[ej[e]])
        if a >= 0:
            lists.setdefault((a, a), []).append((e, 0))
        if b >= 0:
            lists.setdefault((b, b), []).append((e, 1))
        if a >= 0 and b >= 0:
            if a < b:
                lists.setdefault((a, b), []).append((e, 1 if flip_side_when_a_below_b else 0))
            else:
                lists.setdefault((b, a), []).append((e, 1))
    return lists


def assemble_f64(J, err, ei, ej, sys_idx, nV, lam, want_H=True, flip_side_when_a_below_b=False):
    """k_ess_assemble in float64, operation for operation: per entry h = sum over k = 0..6 of
    Ja[k][r] Jb[k][c] in that order, acc += h over the pair's entries in edge order, + lambda on the
    diagonal; b: g = sum over k of Ja[k][r] e[k], acc -= g.  J: nE x 2 x 7 x 7 ([side][k][d]); only
    blocks of system vertices are read.  -> (H upper triangle, lower zero; or None), b"""
    n = 7 * nV
    H = np.zeros((n, n)) if want_H else None
    bv = np.zeros(n)
    for (a, b), ents in gather_lists(ei, ej, sys_idx, nV, flip_side_when_a_below_b).items():
        if a == b:
            g_acc = np.zeros(7)
            for e, s in ents:
                g = np.zeros(7)
                for k in range(7):
                    g = g + J[e, s, k, :] * err[e, k]
                g_acc = g_acc - g
            bv[7 * a:7 * a + 7] = g_acc
        if not want_H:
            continue
        acc = np.zeros((7, 7))
        for e, s in ents:
            Ja, Jb = J[e, s], J[e, s if a == b else 1 - s]
            h = np.zeros((7, 7))
            for k in range(7):
                h = h + np.outer(Ja[k], Jb[k])
            acc = acc + h
        if a == b:
            acc[np.diag_indices(7)] += lam
            acc = np.triu(acc)
        H[7 * a:7 * a + 7, 7 * b:7 * b + 7] = acc
    return H, bv


def csum(v):
    """ora_csum (oracle/ba.c): chunks of 64, each by the tree a[i] += a[i + off], off = 32 .. 1, zero
    padded; recursively over the chunk totals; a single term is returned untouched"""
    v = np.array(v, np.float64)
    if len(v) == 0:
        return 0.0
    while len(v) > 1:
        m = (len(v) + 63) // 64
        a = np.zeros((m, 64))
        a.reshape(-1)[:len(v)] = v
        off = 32
        while off >= 1:
            a[:, :off] = a[:, :off] + a[:, off:2 * off]
            off >>= 1
        v = a[:, 0].copy()
    return float(v[0])
