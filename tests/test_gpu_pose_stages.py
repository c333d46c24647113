"""One linearisation and one LM trial of PoseOptimization on the device, stage by stage, through
orbgpu_unit_pose_stage (k_pose_stage: k_pose_opt's own device functions), each intermediate held
to what defines it:

  T0, err, chi2e, rho, T_trial, the trial's chi2e and rho, the float pose
                      50 digits (pose_mp.py) at the device's own inputs: E_gpu <= 8 E_64 + 8 * 2^-52
  J                   the exact central differences: error <= 8 x the float64 restatement's own;
                      the monocular third row is bit-zero
  chi2e, terms        bit for bit the NumPy float64 restatement on the device's own J and err, in the
                      kernel's operation order
  the 28 sums, the trial's sum of rho, scale
                      bit for bit ora_csum of the device's own terms; every output bit-equal between
                      256 and 512 threads
  x                   backward error <= max(8 x LAPACK's, 6 * 2^-53) on the device's own H + lambda I, b
  classification chi2 the float32 of the device's own double chi2, bit for bit

E is the largest distance to the 50-digit value over the case's active edges (vectors scaled by
max(1, |ref|_inf)), E_64 that of the float64 restatement at the same inputs.  Cases and their
conditions: pose_stage_cases.py, test_pose_mp_cpu.py.  The LM control (rho, the lambda update,
nBadLM) is not here: it stays pinned bit for bit to the oracle by test_gpu_pose.py."""
import functools

import numpy as np
import pytest

import pose_mp as pm
import pose_stage_cases as pc
from essgraph_cases import csum
from pose_units import stage, stage_of

pytestmark = pytest.mark.gpu
mp = pm.mp
DIAG = [0, 6, 11, 15, 18, 20]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _active(name):
    return np.flatnonzero((pc.case(name)[1] & 1) == 0)


def _report(label, E_gpu, E_64):
    for k in E_64:
        print("%s %-6s E_gpu %.3e  E_64 %.3e  ratio %.2f" % (label, k, E_gpu[k], E_64[k],
                                                             E_gpu[k] / E_64[k] if E_64[k] else (0.0 if E_gpu[k] == 0 else np.inf)))


@functools.lru_cache(maxsize=None)
def _edge_refs(name):
    """(50-digit reference, float64 restatement) of the active edges at the device's own T0"""
    o = stage_of(name)
    ed, _ = pc.edges(name)
    return ([pm.edge_reference(o["T0"], ed[k], pc.cam(name)) for k in _active(name)],
            [pm.edge_f64(o["T0"], ed[k], pc.cam(name)) for k in _active(name)])


# ---------------------------------------------------------------- structure and the estimate
@pytest.mark.parametrize("threads", [256, 512])
@pytest.mark.parametrize("name", pc.ALL_CASES)
def test_structure_and_estimate(gpu, name, threads):
    pr, fl = pc.case(name)
    o = stage_of(name, "init", threads)
    act = _active(name)
    assert o["ne"] == len(fl) and o["nA"] == len(act) and o["ok"] == 1
    assert np.array_equal(o["keypoint"], np.flatnonzero(pr["has_mp"]))
    inact = np.setdiff1d(np.arange(len(fl)), act)
    for k in ("err", "chi2e", "rho", "J", "terms", "chi2e_trial", "rho_trial"):
        assert np.all(np.isfinite(o[k][act])) and np.all(np.isnan(o[k][inact])), k
    ref, arm = pm.from_Tcw(pr["Tcw"])
    assert name not in pc.ARMS or arm == pc.ARMS[name]
    E_gpu = pm.se3_errors([o["T0"]], [ref])
    E_64 = pm.se3_errors(pm.f64("from_Tcw", [pr["Tcw"].reshape(16)]), [ref])
    _report("%s T0 (arm %d)" % (name, arm), E_gpu, E_64)
    assert o["T0"][3] >= 0 and pm.within_bound(E_gpu, E_64)


# ---------------------------------------------------------------- the edges against 50 digits
@pytest.mark.parametrize("name", pc.MP_CASES)
def test_errors_and_jacobians(gpu, name):
    o = stage_of(name)
    act = _active(name)
    refs, f = _edge_refs(name)
    gpu_rows = [dict(err=o["err"][k], chi2=o["chi2e"][k], rho=o["rho"][k], J=o["J"][k]) for k in act]
    keys = ("err", "chi2", "rho", "J")
    E_gpu, E_64 = pm.edge_errors(gpu_rows, refs, keys), pm.edge_errors(f, refs, keys)
    _report(name, E_gpu, E_64)
    print("%s J noise ratio %.2f" % (name, E_gpu["J"] / E_64["J"]))
    assert pm.within_bound({k: E_gpu[k] for k in ("err", "chi2", "rho")}, {k: E_64[k] for k in ("err", "chi2", "rho")})
    assert E_gpu["J"] <= 8 * E_64["J"]
    ed, _ = pc.edges(name)
    mono = np.array([not ed[k].stereo for k in act])
    assert not _bits(o["J"][act][mono][:, 12:]).any() and not _bits(o["err"][act][mono][:, 2]).any()
    assert np.all(o["J"][act][~mono][:, 12:14] != 0)
    # the robust chi2 took the side of delta^2 the reference takes
    for k, r in zip(act, refs):
        assert (o["rho"][k] == o["chi2e"][k]) == (r["rho"] == r["chi2"])


@pytest.mark.parametrize("lam_kind", ["init", "x1000"])
@pytest.mark.parametrize("name", pc.MP_CASES)
def test_trial(gpu, name, lam_kind):
    o = stage_of(name, lam_kind)
    assert o["ok"] == 1
    x = o["x"]
    theta = mp.sqrt(sum(mp.mpf(float(v)) ** 2 for v in x[:3]))
    assert pm.threshold_margin(theta) >= 1e-6       # the device's step does not sit on exp's threshold
    ref = pm.to_row(pm.mul(pm.exp(x), pm.from_row(o["T0"])))
    E_gpu, E_64 = pm.se3_errors([o["T_trial"]], [ref]), pm.se3_errors([pm.trial64(x, o["T0"])], [ref])
    _report("%s %s T_trial (theta %.2e)" % (name, lam_kind, float(theta)), E_gpu, E_64)
    assert o["T_trial"][3] >= 0 and pm.within_bound(E_gpu, E_64)
    # the trial's pass at the device's own T_trial
    ed, _ = pc.edges(name)
    act = _active(name)
    refs = [pm.edge_reference(o["T_trial"], ed[k], pc.cam(name), with_J=False) for k in act]
    assert min(float(r["delta_margin"]) for r in refs) >= 1e-6
    assert min([float(r["invz_margin"]) for r in refs if "invz_margin" in r] or [1]) >= 2.0 ** -40
    f = [pm.edge_f64(o["T_trial"], ed[k], pc.cam(name)) for k in act]
    keys = ("chi2", "rho")
    E_gpu = pm.edge_errors([dict(chi2=o["chi2e_trial"][k], rho=o["rho_trial"][k]) for k in act], refs, keys)
    E_64 = pm.edge_errors(f, refs, keys)
    _report("%s %s trial" % (name, lam_kind), E_gpu, E_64)
    assert pm.within_bound(E_gpu, E_64)
    # the float pose of T_trial
    ref16 = [pm.to_Tcw(o["T_trial"])]
    E_gpu = pc.tcw_errors([o["Tcw_trial"]], ref16)
    E_64 = pc.tcw_errors(pm.f64("to_Tcw", [o["T_trial"]]), ref16)
    _report("%s %s Tcw_trial" % (name, lam_kind), E_gpu, E_64)
    assert pm.within_bound(E_gpu, E_64)
    assert np.array_equal(o["Tcw_trial"][12:], np.float32([0, 0, 0, 1]))


# ---------------------------------------------------------------- bit for bit: chi2, terms, sums
def _edge_arrays(name):
    ed, _ = pc.edges(name)
    return (np.array([e.info for e in ed]), np.array([e.delta for e in ed]), np.array([e.robust for e in ed]),
            np.array([e.stereo for e in ed]))


@pytest.mark.parametrize("name", pc.ALL_CASES)
def test_terms_bit_for_bit(gpu, name):
    o = stage_of(name)
    act = _active(name)
    info, delta, robust, stereo = (a[act] for a in _edge_arrays(name))
    err, J, c = o["err"][act], o["J"][act], o["chi2e"][act]
    assert np.array_equal(_bits(pm.chi2_in_kernel_order(err, info, stereo)), _bits(c))
    t = pm.terms_in_kernel_order(J, err, c, info, delta, robust)
    assert np.array_equal(_bits(t), _bits(o["terms"][act]))
    assert np.array_equal(_bits(o["rho"][act]), _bits(o["terms"][act][:, 0]))
    rt = pm.terms_in_kernel_order(J, err, o["chi2e_trial"][act], info, delta, robust)[:, 0]
    assert np.array_equal(_bits(rt), _bits(o["rho_trial"][act]))


@pytest.mark.parametrize("name", pc.ALL_CASES)
def test_sums_are_canonical_at_both_widths(gpu, name):
    act = _active(name)
    for lam_kind in ("init", "x1000"):
        o = stage_of(name, lam_kind, 512)
        for q in range(28):
            assert o["sums"][q] == csum(o["terms"][act, q]), q
        assert o["chi2_trial"] == csum(o["rho_trial"][act])
        x, b, lam = o["x"], o["sums"][22:], o["lambda"]
        assert o["scale"] == csum(x * (lam * x + b))
        o2 = stage_of(name, lam_kind, 256)
        for k, v in o.items():
            if not isinstance(v, np.ndarray):
                assert v == o2[k], k
            elif v.dtype == np.int32:
                assert np.array_equal(v, o2[k]), k
            else:   # inactive rows hold the same NaN at both widths
                assert np.array_equal(_bits(v), _bits(o2[k])), k


# ---------------------------------------------------------------- the solve
def _eta(A, x, b):
    L = np.longdouble
    r = np.abs(A.astype(L) @ x.astype(L) - b.astype(L)).max()
    return float(r / (np.abs(A).sum(1).max() * np.abs(x).max() + np.abs(b).max()))


def _system(o):
    H = np.zeros((6, 6))
    H[np.triu_indices(6)] = o["sums"][1:22]
    return H + np.triu(H, 1).T + o["lambda"] * np.eye(6), o["sums"][22:]


@pytest.mark.parametrize("lam_kind", ["init", "x1000"])
@pytest.mark.parametrize("name", pc.ALL_CASES)
def test_solve_backward_error(gpu, name, lam_kind):
    o = stage_of(name, lam_kind)
    A, b = _system(o)
    mx = np.abs(o["sums"][1:22][DIAG]).max()
    assert o["lambda"] == dict(init=1e-5, x1000=1e-2)[lam_kind] * mx
    eta, eta_lapack = _eta(A, o["x"], b), _eta(A, np.linalg.solve(A, b), b)
    print("%s lambda %.3e: eta %.3e, eta_lapack %.3e" % (name, o["lambda"], eta, eta_lapack))
    assert o["ok"] == 1
    assert eta <= max(8 * eta_lapack, 6 * 2.0 ** -53)


@pytest.mark.parametrize("threads", [256, 512])
@pytest.mark.parametrize("name", ["n9", "n65", "compaction", "rot179y", "n513"])
def test_indefinite_system_fails_the_solve(gpu, name, threads):
    """lambda = -2 x the largest diagonal entry: H + lambda I has only negative diagonal entries, the
    factorisation reports failure with every number finite, x stays the solver's untouched zero and
    the trial's pose is exp(0) * T0 as the device computes it"""
    from pose_units import unit_se3
    o = stage_of(name, "negative", threads)
    A, _ = _system(o)
    assert np.all(np.diag(A) < 0) and np.all(np.isfinite(o["sums"]))
    assert o["ok"] == 0 and not _bits(o["x"]).any()
    same = unit_se3("mul", unit_se3("exp", np.zeros((1, 6))), o["T0"][None])[0]
    assert np.array_equal(_bits(o["T_trial"]), _bits(same))
    assert o["scale"] == 0.0 and np.isfinite(o["chi2_trial"])
    act = _active(name)
    assert o["chi2_trial"] == csum(o["rho_trial"][act])


# ---------------------------------------------------------------- the classification's chi2
@pytest.mark.parametrize("name", pc.ALL_CASES)
def test_classification_chi2_is_the_float_of_the_pass(gpu, name):
    for lam_kind in ("init", "x1000"):
        o = stage_of(name, lam_kind)
        act = _active(name)
        assert np.array_equal(_bits(o["chi2_class"][act]), _bits(o["chi2e_trial"][act].astype(np.float32)))
        assert np.all(np.isfinite(o["chi2_class"]))


def test_inactive_edges_are_classified_at_the_trial_pose(gpu):
    """an inactive edge has no pass; its classification chi2 is the float of the reference's chi2 at the
    device's T_trial to within the rule on the double it was rounded from"""
    name = "compaction"
    o = stage_of(name)
    ed, _ = pc.edges(name)
    inact = np.flatnonzero(pc.case(name)[1] & 1)
    refs = [pm.edge_reference(o["T_trial"], ed[k], pc.cam(name), with_J=False) for k in inact]
    f = [pm.edge_f64(o["T_trial"], ed[k], pc.cam(name)) for k in inact]
    f32 = [dict(chi2=float(np.float32(x["chi2"]))) for x in f]
    E_gpu = pm.edge_errors([dict(chi2=float(o["chi2_class"][k])) for k in inact], refs, ("chi2",))
    E_64 = pm.edge_errors(f32, refs, ("chi2",))
    _report("inactive edges' float chi2", E_gpu, E_64)
    assert pm.within_bound(E_gpu, E_64)


# ---------------------------------------------------------------- the entry's argument checks
def test_unit_entry_validates(gpu):
    import ctypes as C

    from c_orb_slam_amd._lib import ORB_E_CAPACITY, ORB_E_INVALID, lib, pose_stage, ptr
    from pose_cases import pose_problem
    from pose_units import problem_struct
    pr, fl = pc.case("n9")
    P, keep = problem_struct(pr)
    S = pose_stage()
    L = lib()
    call = L.orbgpu_unit_pose_stage
    assert call(None, ptr(fl), 1.0, 256, C.byref(S)) == ORB_E_INVALID
    assert call(C.byref(P), None, 1.0, 256, C.byref(S)) == ORB_E_INVALID
    assert call(C.byref(P), ptr(fl), 1.0, 256, None) == ORB_E_INVALID
    assert call(C.byref(P), ptr(fl), 1.0, 128, C.byref(S)) == ORB_E_INVALID
    assert call(C.byref(P), ptr(fl), float("nan"), 256, C.byref(S)) == ORB_E_INVALID
    assert call(C.byref(P), ptr(fl), float("inf"), 512, C.byref(S)) == ORB_E_INVALID
    assert call(C.byref(P), ptr(fl), 1.0, 512, C.byref(S)) == 0 and (S.ne, S.nA, S.ok) == (9, 9, 1)   # every output NULL
    big = pose_problem(1, N=8300, mp_frac=1.0)
    Pb, keepb = problem_struct(big)
    assert call(C.byref(Pb), ptr(np.full(8300, 2, np.uint8)), 1.0, 512, C.byref(S)) == ORB_E_CAPACITY
    o = stage(pr, np.full(9, 3, np.uint8), 1.0)     # no active edge: empty sums, a zero system
    assert o["nA"] == 0 and not o["sums"].any() and np.all(np.isnan(o["chi2e"]))
