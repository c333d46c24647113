"""ctypes callers of the pose graph's test-only entries (include/orbslam_gpu.h): orbgpu_unit_sim3,
orbgpu_unit_essgraph_stage and the orbgpu_unit_set_ess_dense_max knob."""
import contextlib
import ctypes as C

import numpy as np

from c_orb_slam_amd._lib import check, essgraph_problem, essgraph_stage, lib, ptr

SIM3_OPS = dict(exp=(0, 7, 0, 0, 8), log=(1, 8, 0, 0, 7), mul=(2, 8, 8, 0, 8), inverse=(3, 8, 0, 0, 8),
                map=(4, 8, 3, 0, 3), edge_error=(5, 8, 8, 8, 7))   # op, columns of a, b, c, out


def unit_sim3(op, a, b=None, c=None):
    code, ca, cb, cc, co = SIM3_OPS[op]
    arrs = []
    for x, cols in ((a, ca), (b, cb), (c, cc)):
        if cols == 0:
            assert x is None
            arrs.append(None)
            continue
        x = np.ascontiguousarray(x, np.float64)
        assert x.shape == (len(a), cols)
        arrs.append(x)
    out = np.full((len(a), co), np.nan)
    check(lib().orbgpu_unit_sim3(code, len(a), ptr(arrs[0]), ptr(arrs[1]), ptr(arrs[2]), ptr(out)), "orbgpu_unit_sim3")
    return out


def problem_struct(pr):
    """(essgraph_problem, the arrays it points to)"""
    a = dict(Scw=np.ascontiguousarray(pr["Scw"], np.float64),
             Snc=np.ascontiguousarray(pr.get("ScwNonCorrected", pr["Scw"]), np.float64),
             fixed=np.ascontiguousarray(pr["fixed"], np.uint8), ei=np.ascontiguousarray(pr["edge_i"], np.int32),
             ej=np.ascontiguousarray(pr["edge_j"], np.int32), el=np.ascontiguousarray(pr["edge_loop"], np.uint8))
    P = essgraph_problem(len(a["Scw"]), ptr(a["Scw"]), ptr(a["Snc"]), ptr(a["fixed"]), len(a["ei"]), ptr(a["ei"]),
                         ptr(a["ej"]), ptr(a["el"]), int(bool(pr["bFixScale"])), 0, None, None)
    return P, a


def stage(pr, lam, want_H=True):
    """One linearisation and one LM trial at lambda -> dict of every stage output (H None if not wanted)"""
    import essgraph_cases as ec
    P, keep = problem_struct(pr)
    nKF, nE = P.nKF, P.nE
    n = 7 * ec.system_index(pr)[1]
    o = dict(sysIdx=np.full(nKF, -7, np.int32), meas=np.full((nE, 8), np.nan), err=np.full((nE, 7), np.nan),
             chi2e=np.full(nE, np.nan), J=np.full((nE, 2, 7, 7), np.nan), H=np.full((n, n), np.nan) if want_H else None,
             b=np.full(n, np.nan), x_solve=np.full(n, np.nan), x=np.full(n, np.nan), est_trial=np.full((nKF, 8), np.nan),
             chi2e_trial=np.full(nE, np.nan))
    S = essgraph_stage(-9, -9, -9, *(ptr(o[k]) for k in ("sysIdx", "meas", "err", "chi2e", "J", "H", "b", "x_solve", "x",
                                                         "est_trial", "chi2e_trial")), 0.0, 0.0, 0.0)
    check(lib().orbgpu_unit_essgraph_stage(C.byref(P), float(lam), C.byref(S)), "orbgpu_unit_essgraph_stage")
    assert S.nV * 7 == n
    o.update(solver=S.solver, nV=S.nV, ok=S.ok, chi2=S.chi2, chi2_trial=S.chi2_trial, scale=S.scale, n=n)
    return o


@contextlib.contextmanager
def ess_dense_max(rows):
    """the dense solver's row limit lowered for the block's duration (0: every system is tiled)"""
    assert lib().orbgpu_unit_set_ess_dense_max(rows) == 0
    try:
        yield
    finally:
        assert lib().orbgpu_unit_set_ess_dense_max(144) == 0
