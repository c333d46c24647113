"""The frames of the pose stage tests (orbgpu_unit_pose_stage) and the input batches of the SE3 unit
tests (orbgpu_unit_se3): small problems built from pose_cases.pose_problem.

A case is (problem, flags): flags holds one byte per edge (bit 0 inactive, bit 1 robust kernel set),
edges being the rows with a map point in keypoint order.  Cases in MP_CASES have at most 130 edges
and are compared with the 50-digit reference (pose_mp.py); the larger ones get the bit-for-bit
checks only.  test_pose_mp_cpu.py checks the conditions the comparisons rest on (no chi2 near
Huber's delta^2, no stereo 1/p_z near a float32 rounding midpoint, no theta near exp's threshold)
for the seeds committed here.
"""
import functools
import math

import numpy as np

import pose_mp as pm
from pose_cases import pose_problem

# active-edge counts: one chunk of 64, a partial chunk, one and two edges per thread at 256 and 512
# threads, more than one level of the chunk totals (4097 = 64 chunks + 1), the capacity
COUNTS = (3, 9, 10, 63, 64, 65, 255, 256, 257, 511, 512, 513, 4097, 8192)


def _axis_rot(axis, deg):
    a = np.zeros(3)
    a[axis] = 1.0
    th = math.radians(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * K @ K


def repose(pr, R_new, t_new):
    """the same camera-frame points and observations seen from the pose (R_new, t_new)"""
    T = pr["Tcw"].astype(np.float64)
    Xc = pr["Xw"].astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    pr = dict(pr)
    pr["Xw"] = ((Xc - t_new) @ R_new).astype(np.float32)
    Tn = np.eye(4)
    Tn[:3, :3], Tn[:3, 3] = R_new, t_new
    pr["Tcw"] = Tn.astype(np.float32)
    return pr


def _flags(n, robust=True, every_second_inactive=False):
    f = np.full(n, 2 if robust else 0, np.uint8)
    if every_second_inactive:
        f[1::2] |= 1
    return f


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (problem, flags)"""
    if name[1:].isdigit():                                    # nK: K edges, all active, mixed
        n = int(name[1:])
        return pose_problem(100 + n, N=n, mp_frac=1.0, outlier_frac=0.2), _flags(n)
    if name == "compaction":                                  # 130 edges, every second one inactive
        return pose_problem(41, N=130, mp_frac=1.0, outlier_frac=0.2), _flags(130, every_second_inactive=True)
    if name == "sparse":                                      # rows without a map point between the edges
        pr = pose_problem(42, N=90, mp_frac=0.5, outlier_frac=0.2)
        return pr, _flags(int(pr["has_mp"].sum()))
    if name in ("mono", "stereo", "alternating", "no_robust", "robust_mixed"):
        pr = pose_problem(50, N=40, mp_frac=1.0, outlier_frac=0.3,
                          stereo_frac=dict(mono=0.0, stereo=1.0).get(name, 0.6))
        if name == "alternating":
            pr["obs"][1::2, 2] = -1.0
            pr["obs"][0::2, 2] = np.where(pr["obs"][0::2, 2] < 0, pr["obs"][0::2, 0] - 5.0, pr["obs"][0::2, 2])
        f = _flags(40, robust=name != "no_robust")
        if name == "robust_mixed":
            f[::3] = 0
        return pr, f
    rng = np.random.default_rng(7)
    pr = pose_problem(60, N=24, mp_frac=1.0, outlier_frac=0.25)
    t = rng.normal(0, 2.0, 3)
    if name == "identity":
        return repose(pr, np.eye(3), np.zeros(3)), _flags(24)
    if name == "float_R":                                     # the float rounding of a rotation, as SetPose leaves it
        return pr, _flags(24)
    axis = dict(rot179x=0, rot179y=1, rot179z=2)[name]
    return repose(pr, _axis_rot(axis, 179.0), t), _flags(24)


COUNT_CASES = tuple("n%d" % n for n in COUNTS)
MIX_CASES = ("mono", "stereo", "alternating", "no_robust", "robust_mixed", "compaction", "sparse")
POSE_CASES = ("float_R", "identity", "rot179x", "rot179y", "rot179z")
ARMS = dict(float_R=0, identity=0, rot179x=1, rot179y=2, rot179z=3)
MP_CASES = tuple(c for c in COUNT_CASES if int(c[1:]) <= 130) + MIX_CASES + POSE_CASES
ALL_CASES = COUNT_CASES + MIX_CASES + POSE_CASES


def edges(name):
    """the case's edges (pose_mp.Edge) in edge order and their keypoint indices"""
    pr, fl = case(name)
    kp = np.flatnonzero(pr["has_mp"])
    return [pm.Edge(pr["Xw"][i], pr["obs"][i], pr["inv_sigma2"][i], fl[k] & 2) for k, i in enumerate(kp)], kp


def cam(name):
    return [float(v) for v in case(name)[0]["cam"]]


# ---------------------------------------------------------------- orbgpu_unit_se3's batches
N_ITEMS = 261   # more than one 256-thread block and no multiple of it
PI = float(pm.mp.pi)
THETA = {"T1e-7": 1e-7, "Tbelow": 1e-5 * (1 - 1e-3), "Tabove": 1e-5 * (1 + 1e-3), "T8e-5": 8e-5, "T1e-3": 1e-3,
         "T0.1": 0.1, "T1": 1.0, "T2.5": 2.5, "Tpi": PI}
AXIS_THETAS = ("T0.1", "T2.5", "Tpi")


@functools.lru_cache(maxsize=None)
def exp_inputs():
    """class -> u (N_ITEMS x 6): |omega| = the class's angle (to within rounding), |upsilon| log-uniform
    in [0.01, 10]; the 'axis' classes rotate about +-x, +-y, +-z in turn (Eigen's three diagonal arms
    beyond 2 pi / 3).  T8e-5 separates a threshold of 1e-4 from g2o's 1e-5."""
    out = {}
    for c, (tn, th) in enumerate(THETA.items()):
        rng = np.random.default_rng(3000 + c)
        w = rng.standard_normal((N_ITEMS, 3))
        w *= th / np.linalg.norm(w, axis=1, keepdims=True)
        v = rng.standard_normal((N_ITEMS, 3))
        v *= 10.0 ** rng.uniform(-2, 1, (N_ITEMS, 1)) / np.linalg.norm(v, axis=1, keepdims=True)
        out[tn] = np.concatenate([w, v], 1)
    for c, tn in enumerate(AXIS_THETAS):
        rng = np.random.default_rng(4000 + c)
        k = np.arange(N_ITEMS)
        w = np.zeros((N_ITEMS, 3))
        w[k, k % 3] = THETA[tn] * np.where((k // 3) % 2, -1.0, 1.0)
        out["axis_" + tn] = np.concatenate([w, rng.uniform(-10, 10, (N_ITEMS, 3))], 1)
    return out


@functools.lru_cache(maxsize=None)
def exp_reference(name):
    """rows of 7 mpf, and Eigen's matrix -> quaternion arm of each item"""
    S = [pm.exp(u) for u in exp_inputs()[name]]
    return [pm.to_row(s) for s in S], [pm.sm.quat_from_R(s[0])[1] for s in S]


def _se3_rows(rng, n):
    q = rng.standard_normal((n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return np.concatenate([q, rng.uniform(-100, 100, (n, 3))], 1)


@functools.lru_cache(maxsize=None)
def group_inputs():
    rng = np.random.default_rng(78)
    return dict(a=_se3_rows(rng, N_ITEMS), b=_se3_rows(rng, N_ITEMS), X=rng.uniform(-1e3, 1e3, (N_ITEMS, 3)))


@functools.lru_cache(maxsize=None)
def group_reference(op):
    g = group_inputs()
    a, b = [pm.from_row(r) for r in g["a"]], [pm.from_row(r) for r in g["b"]]
    if op == "mul":
        return [pm.to_row(pm.mul(x, y)) for x, y in zip(a, b)]
    return [pm.smap(x, X) for x, X in zip(a, g["X"])]


@functools.lru_cache(maxsize=None)
def tcw_inputs():
    """float Tcw (n x 16): random rotations (trace > 0 and < 0), 179 degrees about x, y, z with a small
    random tilt, the identity; every R is the float rounding of a rotation, so not exactly orthonormal"""
    rng = np.random.default_rng(79)
    out = []
    for k in range(N_ITEMS):
        kind = k % 6
        if kind == 5:
            R = np.eye(3)
        elif kind >= 2:
            w = rng.normal(0, 0.005, 3)
            R = pm.exp64(np.concatenate([w, np.zeros(3)]))[0] @ _axis_rot(kind - 2, 179.0)
        else:
            w = rng.standard_normal(3)
            w *= (rng.uniform(0.01, 1.5) if kind == 0 else rng.uniform(2.2, 3.1)) / np.linalg.norm(w)
            R = pm.exp64(np.concatenate([w, np.zeros(3)]))[0]
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = R, rng.uniform(-50, 50, 3)
        out.append(T.reshape(16))
    return np.array(out, np.float32)


@functools.lru_cache(maxsize=None)
def tcw_reference():
    """(rows of 7 mpf, arms) of toSE3Quat on tcw_inputs()"""
    r = [pm.from_Tcw(T) for T in tcw_inputs()]
    return [x[0] for x in r], [x[1] for x in r]


@functools.lru_cache(maxsize=None)
def to_tcw_inputs():
    """rows of 7 float64: the restatement's toSE3Quat of tcw_inputs()"""
    return pm.f64("from_Tcw", tcw_inputs())


@functools.lru_cache(maxsize=None)
def to_tcw_reference():
    return [pm.to_Tcw(r) for r in to_tcw_inputs()]


def tcw_errors(out, ref):
    """largest |out - ref| over the 16 entries, translation column scaled by max(1, |t_ref|_inf)"""
    E = dict(R=0.0, t=0.0)
    for o, r in zip(np.asarray(out, np.float64).reshape(-1, 16), ref):
        idx_t = (3, 7, 11)
        sc = max(1, max(abs(r[i]) for i in idx_t))
        E["t"] = max(E["t"], float(max(abs(pm._f(o[i]) - r[i]) for i in idx_t) / sc))
        E["R"] = max(E["R"], float(max(abs(pm._f(o[i]) - r[i]) for i in range(16) if i not in idx_t)))
    return E


# ---------------------------------------------------------------- the oracle frames of test_gpu_pose.py
def negative_depth_frame():
    """about 10 % of the points behind the camera (mirrored through the camera centre), all finite"""
    pr = pose_problem(5, N=300, mp_frac=1.0)
    T = pr["Tcw"].astype(np.float64)
    Xc = pr["Xw"].astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    back = np.random.default_rng(5).random(300) < 0.1
    Xc[back] = -Xc[back]
    pr["Xw"] = ((Xc - T[:3, 3]) @ T[:3, :3]).astype(np.float32)
    pr["behind"] = back
    return pr


def degenerate_depth_frame():
    """identity pose, depths of at least 4, then p_z = 0 exactly (row 5), p_z = -3 (row 9) and
    Xw = (0, 0, 0) (row 20)"""
    pr = pose_problem(3, N=64, mp_frac=1.0)
    T = pr["Tcw"].astype(np.float64)
    Xc = pr["Xw"].astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    Xc[:, 2] = np.maximum(Xc[:, 2], 4.0)
    pr["Tcw"] = np.eye(4, dtype=np.float32)
    pr["Xw"] = Xc.astype(np.float32)
    pr["Xw"][5, 2] = 0.0
    pr["Xw"][9, 2] = -3.0
    pr["Xw"][20] = 0.0
    return pr
