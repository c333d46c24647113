"""Optimizer::OptimizeEssentialGraph without a GPU: the NumPy reference's own sanity, the
conditions the GPU test's inputs have to satisfy (asserted on the reference alone), and the C ABI's
argument validation."""
import ctypes as C

import numpy as np
import pytest

import c_orb_slam_amd as orb
import essgraph_cases as ec
from c_orb_slam_amd._lib import ORB_E_INVALID, ORB_E_NODEVICE, lib, ptr


@pytest.mark.parametrize("theta,sigma", [(0.7, 0.3), (1e-7, 0.3), (0.7, 1e-7), (1e-7, 1e-8)])
def test_reference_log_inverts_exp(theta, sigma):
    """log(exp(u)) == u to 1e-12 in each of the four (theta, sigma) branches"""
    rng = np.random.default_rng(0)
    w = rng.standard_normal((64, 3))
    w *= theta * rng.uniform(0.2, 1.0, (64, 1)) / np.linalg.norm(w, axis=1, keepdims=True)
    u = np.concatenate([w, rng.standard_normal((64, 3)), sigma * rng.uniform(-1, 1, (64, 1))], -1)
    assert np.abs(ec.s3_log(ec.s3_exp(u)) - u).max() <= 1e-12


@pytest.mark.parametrize("N,fix", [(12, True), (12, False), (40, True), (40, False)])
def test_reference_recovers_zero_residual_truth(N, fix):
    """every rounding variant of the reference reaches the truth on the GPU test's inputs (with the
    scale free that depends on the seed: essgraph_cases.ZERO_SEEDS)"""
    pr, truth = ec.zero_residual_case(N, fix)
    for variant in range(3):
        r = ec.ref_optimize(pr, 20, variant)
        assert ec.pose_distance(r["Scw"], truth) <= 1e-9
        assert r["chi2"][0] > 1.0 and r["chi2"][-1] <= 1e-18


@pytest.mark.parametrize("name", sorted(ec.RING_CASES))
def test_ring_cases_are_well_conditioned(name):
    """The rounding-only variants of the reference agree far inside the GPU test's tolerances."""
    refs = ec.ring_reference(name)
    ini, fin, pose = ec.variant_spread(refs)
    print(name, "spread: initial chi2 %.2e final chi2 %.2e pose %.2e" % (ini, fin, pose))
    assert ini <= 1e-12
    assert fin <= 1e-6
    assert pose <= 1e-4
    pr = ec.ring_case(name)
    assert ec.pose_distance(refs[0]["Scw"], pr["Scw"]) > 0.5          # the optimisation moves the poses
    assert refs[0]["chi2"][-1] > 1e-3                                # and leaves a residual


def test_reject_case_rejects_early_in_every_variant():
    """The retried-trial case of the GPU test: nine clear rejections, then a clear acceptance, in each
    rounding variant, so the trial count is not noise there."""
    pr, refs = ec.reject_case()
    for r in refs:
        assert r["trials_per_solve"] == [10] and r["n_solves"] == 1
        t = np.array(r["trial_chi2"])
        assert np.all(t[:9] > 1.05 * r["chi2"][0]) and t[9] < 0.95 * r["chi2"][0]
    c1 = np.array([r["chi2"][1] for r in refs])
    assert (c1.max() - c1.min()) / c1.max() <= 1e-3
    assert ec.variant_spread(refs)[2] <= 1e-1


def test_reject_all_case_rejects_ten_trials_in_every_variant():
    pr, refs = ec.reject_all_case()
    for r in refs:
        assert r["trials_per_solve"] == [10] and r["n_solves"] == 1
        assert np.all(np.array(r["trial_chi2"]) > 1.3 * r["chi2"][0])
        assert r["chi2"][1] == r["chi2"][0]
        assert ec.pose_distance(r["Scw"], pr["Scw"]) <= 1e-12


# ---------------------------------------------------------------- C ABI
def _abi_problem(nMP=3):
    from c_orb_slam_amd._lib import essgraph_problem, essgraph_result
    pr = ec.ring_case("n12_fix")
    a = dict(Scw=pr["Scw"].copy(), Snc=pr["ScwNonCorrected"].copy(), fixed=pr["fixed"].copy(), ei=pr["edge_i"].copy(),
             ej=pr["edge_j"].copy(), el=pr["edge_loop"].copy(), mp=np.ones((nMP, 3), np.float32),
             ref=np.zeros(nMP, np.int32), oS=np.zeros((12, 8)), oT=np.zeros((12, 16), np.float32),
             oX=np.zeros((nMP, 3), np.float32), chi=np.zeros(21))
    P = essgraph_problem(12, ptr(a["Scw"]), ptr(a["Snc"]), ptr(a["fixed"]), len(a["ei"]), ptr(a["ei"]), ptr(a["ej"]),
                         ptr(a["el"]), 1, nMP, ptr(a["mp"]), ptr(a["ref"]))
    R = essgraph_result(ptr(a["oS"]), ptr(a["oT"]), ptr(a["oX"]), ptr(a["chi"]), 21, 0, 0)
    return a, P, R


def test_essgraph_symbol_and_python_entry_exist():
    assert hasattr(lib(), "Optimizer_OptimizeEssentialGraph")
    assert callable(orb.OptimizeEssentialGraph)


def test_essgraph_validates_without_device():
    L = lib()
    call = L.Optimizer_OptimizeEssentialGraph
    a, P, R = _abi_problem()
    assert call(None, 20, C.byref(R)) == ORB_E_INVALID
    assert call(C.byref(P), 20, None) == ORB_E_INVALID
    assert call(C.byref(P), -1, C.byref(R)) == ORB_E_INVALID
    for field in ("Scw", "ScwNonCorrected", "fixed", "edge_i", "edge_j", "edge_loop", "mp_pos", "mp_ref"):
        a, P, R = _abi_problem()
        setattr(P, field, None)
        assert call(C.byref(P), 20, C.byref(R)) == ORB_E_INVALID, field
    for field in ("Scw", "Tcw", "mp_pos", "chi2"):
        a, P, R = _abi_problem()
        setattr(R, field, None)
        assert call(C.byref(P), 20, C.byref(R)) == ORB_E_INVALID, field
    for arr, idx, val in (("ei", 3, 12), ("ej", 3, -1), ("ref", 1, 12), ("ref", 1, -2)):   # indices out of range
        a, P, R = _abi_problem()
        a[arr][idx] = val
        assert call(C.byref(P), 20, C.byref(R)) == ORB_E_INVALID, (arr, val)
    a, P, R = _abi_problem()
    a["ej"][5] = a["ei"][5]                                                               # self edge
    assert call(C.byref(P), 20, C.byref(R)) == ORB_E_INVALID
    for arr, pos, val in (("Scw", (2, 5), np.nan), ("Snc", (4, 0), np.inf), ("Scw", (3, 7), 0.0),
                          ("Snc", (3, 7), -1.0)):                                        # non-finite, s <= 0
        a, P, R = _abi_problem()
        a[arr][pos] = val
        assert call(C.byref(P), 20, C.byref(R)) == ORB_E_INVALID, (arr, pos, val)
    a, P, R = _abi_problem()
    a["mp"][1, 2] = np.nan
    assert call(C.byref(P), 20, C.byref(R)) == ORB_E_INVALID
    a, P, R = _abi_problem()
    if not orb.device_available():   # a valid problem: no CPU fallback
        assert call(C.byref(P), 20, C.byref(R)) == ORB_E_NODEVICE
        with pytest.raises(orb.OrbGpuError) as ei:
            orb.OptimizeEssentialGraph(ec.ring_case("n12_fix"))
        assert ei.value.code == ORB_E_NODEVICE
