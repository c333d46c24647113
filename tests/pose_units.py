"""ctypes callers of PoseOptimization's test-only entries (include/orbslam_gpu.h): orbgpu_unit_se3 and
orbgpu_unit_pose_stage."""
import ctypes as C
import functools

import numpy as np

from c_orb_slam_amd._lib import check, lib, pose_problem, pose_stage, ptr

# op, dtype and columns of a, columns of b (float64), dtype and columns of out
SE3_OPS = dict(exp=(0, np.float64, 6, 0, np.float64, 7), mul=(1, np.float64, 7, 7, np.float64, 7),
               map=(2, np.float64, 7, 3, np.float64, 3), from_Tcw=(3, np.float32, 16, 0, np.float64, 7),
               to_Tcw=(4, np.float64, 7, 0, np.float32, 16))


def unit_se3(op, a, b=None):
    code, ta, ca, cb, to, co = SE3_OPS[op]
    a = np.ascontiguousarray(a, ta)
    assert a.shape == (len(a), ca)
    if cb:
        b = np.ascontiguousarray(b, np.float64)
        assert b.shape == (len(a), cb)
    else:
        assert b is None
    out = np.full((len(a), co), np.nan, to)
    check(lib().orbgpu_unit_se3(code, len(a), ptr(a), ptr(b), ptr(out)), "orbgpu_unit_se3")
    return out


def problem_struct(pr):
    """(pose_problem, the arrays it points to)"""
    a = dict(Tcw=np.ascontiguousarray(pr["Tcw"], np.float32).reshape(16), has_mp=np.ascontiguousarray(pr["has_mp"], np.uint8),
             Xw=np.ascontiguousarray(pr["Xw"], np.float32), obs=np.ascontiguousarray(pr["obs"], np.float32),
             isig=np.ascontiguousarray(pr["inv_sigma2"], np.float32))
    P = pose_problem(len(a["has_mp"]), ptr(a["Tcw"]), ptr(a["has_mp"]), ptr(a["Xw"]), ptr(a["obs"]), ptr(a["isig"]),
                     *[float(v) for v in pr["cam"]])
    return P, a


def stage(pr, flags, lam, threads=512):
    """One linearisation and one LM trial at lambda -> dict of every stage output"""
    P, keep = problem_struct(pr)
    ne = int(keep["has_mp"].sum())
    flags = np.ascontiguousarray(flags, np.uint8)
    assert flags.shape == (ne,)
    f8 = np.float64
    o = dict(keypoint=np.full(ne, -7, np.int32), T0=np.full(7, np.nan), err=np.full((ne, 3), np.nan),
             chi2e=np.full(ne, np.nan), rho=np.full(ne, np.nan), J=np.full((ne, 18), np.nan),
             terms=np.full((ne, 28), np.nan), sums=np.full(28, np.nan), x=np.full(6, np.nan),
             T_trial=np.full(7, np.nan), chi2e_trial=np.full(ne, np.nan), rho_trial=np.full(ne, np.nan),
             chi2_class=np.full(ne, np.nan, np.float32), Tcw_trial=np.full(16, np.nan, np.float32))
    assert all(v.dtype in (f8, np.float32, np.int32) for v in o.values())
    S = pose_stage(-9, -9, -9, *(ptr(o[k]) for k in ("keypoint", "T0", "err", "chi2e", "rho", "J", "terms", "sums", "x",
                                                     "T_trial", "chi2e_trial", "rho_trial", "chi2_class", "Tcw_trial")),
                   0.0, 0.0)
    check(lib().orbgpu_unit_pose_stage(C.byref(P), ptr(flags), float(lam), int(threads), C.byref(S)),
          "orbgpu_unit_pose_stage")
    o.update(ne=S.ne, nA=S.nA, ok=S.ok, chi2_trial=S.chi2_trial, scale=S.scale, **{"lambda": float(lam)})
    return o


LAMBDA_KINDS = ("init", "x1000", "negative")


@functools.lru_cache(maxsize=None)
def stage_of(name, lam_kind="init", threads=512):
    """the stage of pose_stage_cases.case(name) at lambda = 1e-5 x the largest diagonal entry of the
    device's own H (the engine's initial value), 1e3 x that, or -2 x the largest diagonal entry
    (an indefinite H + lambda I: the solve reports failure)"""
    import pose_stage_cases as pc
    pr, fl = pc.case(name)
    H = stage(pr, fl, 1.0, threads)["sums"][1:22]
    mx = np.abs(H[[0, 6, 11, 15, 18, 20]]).max()
    return stage(pr, fl, dict(init=1e-5 * mx, x1000=1e-2 * mx, negative=-2.0 * mx)[lam_kind], threads)
