"""Optimizer::OptimizeEssentialGraph (Optimizer.cc:781-1044) on the GPU against the NumPy float64
reference of essgraph_cases.py.

g2o's numeric Jacobians (delta 1e-9) make the reference itself only defined to about 1e-5 in pose
after an LM step that leaves a residual, so the parity checks are: the initial chi2 (no Jacobian
involved) to 1e-12; zero-residual graphs (where the Jacobian noise is multiplied by b -> 0) to
1e-8 of the ground truth; ring graphs to 10 x the spread between reference evaluations that differ
only in rounding.  Iteration counts are never compared: near convergence accept / reject is noise.

Sizes: N = 12 -> 77 rows, the dense solver; N = 40 -> 273 rows, 5 tiles, the block-sparse solver;
N = 160 -> 1,113 rows, 18 tiles, several dissection levels.
"""
import numpy as np
import pytest

import essgraph_cases as ec

pytestmark = pytest.mark.gpu


def _run(pr, nIterations=20):
    from c_orb_slam_amd import OptimizeEssentialGraph
    return OptimizeEssentialGraph(pr, nIterations)


# ---------------------------------------------------------------- 1. nIterations = 0
@pytest.mark.parametrize("name", sorted(ec.RING_CASES))
def test_initial_chi2_and_identity(gpu, name):
    pr = ec.ring_case(name)
    out = _run(pr, 0)
    ref = ec.ring_reference(name)[0]["chi2"][0]
    rel = abs(out["chi2"][0] - ref) / ref
    print(name, "initial chi2 gpu %.17g ref %.17g rel %.2e" % (out["chi2"][0], ref, rel))
    assert len(out["chi2"]) == 1 and out["n_solves"] == 0 and out["lm_trials"] == 0
    assert rel <= 1e-12
    assert np.array_equal(out["Scw"].view(np.uint64), np.ascontiguousarray(pr["Scw"]).view(np.uint64))


# ---------------------------------------------------------------- 2. zero-residual graphs
@pytest.mark.parametrize("fix", [True, False])
@pytest.mark.parametrize("N", [12, 40, 160])
def test_zero_residual_recovers_truth(gpu, N, fix):
    pr, truth = ec.zero_residual_case(N, fix)
    out = _run(pr, 20)
    dist = ec.pose_distance(out["Scw"], truth)
    print("N=%d fix=%d: distance to truth %.2e, chi2 %.3e -> %.3e, %d solves %d trials"
          % (N, fix, dist, out["chi2"][0], out["chi2"][-1], out["n_solves"], out["lm_trials"]))
    assert out["chi2"][0] > 1.0
    assert dist <= 1e-8
    assert out["chi2"][-1] <= 1e-15
    assert 1 <= out["n_solves"] <= 20


# ---------------------------------------------------------------- 3. ring cases
@pytest.mark.parametrize("name", sorted(ec.RING_CASES))
def test_ring_matches_reference(gpu, name):
    pr = ec.ring_case(name)
    refs = ec.ring_reference(name)
    _, _, spread = ec.variant_spread(refs)
    out = _run(pr, 20)
    rel = abs(out["chi2"][-1] - refs[0]["chi2"][-1]) / refs[0]["chi2"][-1]
    dist = ec.pose_distance(out["Scw"], refs[0]["Scw"])
    bound = 10 * max(spread, 1e-6)
    print("%s: final chi2 gpu %.12g ref %.12g rel %.2e; pose distance %.2e (bound %.2e, variant spread %.2e); "
          "%d solves %d trials" % (name, out["chi2"][-1], refs[0]["chi2"][-1], rel, dist, bound, spread,
                                   out["n_solves"], out["lm_trials"]))
    assert rel <= 1e-6
    assert dist <= bound
    assert np.all(np.diff(out["chi2"]) <= 0)
    assert 1 <= out["n_solves"] <= 20 and len(out["chi2"]) == out["n_solves"] + 1


def test_rejected_trials_are_retried_from_the_linearisation_point(gpu):
    """The first Gauss-Newton step overshoots: nine trials are rejected and retried with a larger
    lambda before one is accepted (test_essgraph_cpu.py asserts that on the reference, with margins
    of more than 5 % of chi2, so the count is not noise here).  Each retry solves with the b of the
    linearisation point.  The accepted step is ill-conditioned: the reference's four rounding
    variants (essgraph_cases.reject_case) differ by 1.3e-4 in chi2 after it; the GPU is held to
    10 x their spread, as the ring cases are."""
    pr, refs = ec.reject_case()
    _, fin, spread = ec.variant_spread(refs)
    out = _run(pr, 20)
    rel = abs(out["chi2"][1] - refs[0]["chi2"][1]) / refs[0]["chi2"][1]
    dist = ec.pose_distance(out["Scw"], refs[0]["Scw"])
    print("reject case: chi2 gpu %s ref %s rel %.2e (variant spread %.2e); pose distance %.2e (spread %.2e); "
          "%d solves %d trials" % (out["chi2"], refs[0]["chi2"], rel, fin, dist, spread, out["n_solves"],
                                   out["lm_trials"]))
    assert out["n_solves"] == 1 and out["lm_trials"] == 10 and out["lm_trials"] > out["n_solves"]
    assert abs(out["chi2"][0] - refs[0]["chi2"][0]) <= 1e-12 * refs[0]["chi2"][0]
    assert rel <= 10 * max(fin, 1e-6)
    assert dist <= 10 * max(spread, 1e-6)
    assert out["chi2"][1] < out["chi2"][0]


def test_ten_rejected_trials_restore_the_estimates(gpu):
    """Every trial of the first iteration overshoots (by more than 30 % of chi2 in every reference
    variant): ten retries, then the optimiser stops with the estimates it started from."""
    pr, refs = ec.reject_all_case()
    out = _run(pr, 20)
    print("reject-all case: chi2 gpu %s ref %s; %d solves %d trials" % (out["chi2"], refs[0]["chi2"], out["n_solves"],
                                                                        out["lm_trials"]))
    assert out["n_solves"] == 1 and out["lm_trials"] == 10
    assert abs(out["chi2"][0] - refs[0]["chi2"][0]) <= 1e-12 * refs[0]["chi2"][0]
    assert out["chi2"][1] == out["chi2"][0]
    assert np.array_equal(out["Scw"].view(np.uint64), np.ascontiguousarray(pr["Scw"]).view(np.uint64))


# ---------------------------------------------------------------- 4. structure edge cases (N = 12)
def _check_against_reference(pr):
    refs = tuple(ec.ref_optimize(pr, 20, v) for v in range(3))
    _, _, spread = ec.variant_spread(refs)
    out = _run(pr, 20)
    rel = abs(out["chi2"][-1] - refs[0]["chi2"][-1]) / refs[0]["chi2"][-1]
    dist = ec.pose_distance(out["Scw"], refs[0]["Scw"])
    print("final chi2 rel %.2e, pose distance %.2e, variant spread %.2e" % (rel, dist, spread))
    assert abs(out["chi2"][0] - refs[0]["chi2"][0]) <= 1e-12 * refs[0]["chi2"][0]
    assert rel <= 1e-6 and dist <= 10 * max(spread, 1e-6)
    return out


def test_duplicated_vertex_pair_is_summed(gpu):
    pr = dict(ec.ring_case("n12_fix"))
    k = [len(pr["edge_i"]) - 1, 9, 9]   # two edges repeated, one of them twice
    for f in ("edge_i", "edge_j", "edge_loop"):
        pr[f] = np.concatenate([pr[f], pr[f][k]])
    # and a normal edge on a pair that a loop edge joins already (a parent edge plus a loop edge)
    pr["edge_i"] = np.append(pr["edge_i"], np.int32(11))
    pr["edge_j"] = np.append(pr["edge_j"], np.int32(0))
    pr["edge_loop"] = np.append(pr["edge_loop"], np.uint8(0))
    out = _check_against_reference(pr)
    single = _run(ec.ring_case("n12_fix"), 20)
    assert ec.pose_distance(out["Scw"], single["Scw"]) > 1e-3   # the duplicates carry weight


def test_edge_between_fixed_vertices_counts_in_chi2_only(gpu):
    pr = dict(ec.ring_case("n12_free"))
    pr["fixed"] = pr["fixed"].copy()
    pr["fixed"][1] = 1   # edge 1 -> 0 now joins two fixed vertices
    Snc = pr["ScwNonCorrected"].copy()
    Snc[1, 4:7] += 0.05   # give that edge a residual: the measurement no longer matches the estimates
    pr["ScwNonCorrected"] = Snc
    out = _check_against_reference(pr)
    assert np.array_equal(out["Scw"][:2], pr["Scw"][:2])
    assert out["chi2"][-1] > 1e-3


def test_free_vertex_without_edge_is_untouched(gpu):
    base = ec.ring_case("n12_fix")
    pr = dict(base)
    extra = base["Scw"][5:6].copy()
    extra[0, 4:7] += 1.0
    pr["Scw"] = np.concatenate([base["Scw"], extra])
    pr["ScwNonCorrected"] = np.concatenate([base["ScwNonCorrected"], extra])
    pr["fixed"] = np.concatenate([base["fixed"], [0]]).astype(np.uint8)
    out = _run(pr, 20)
    assert np.array_equal(out["Scw"][12].view(np.uint64), extra[0].view(np.uint64))
    ref = _run(base, 20)
    assert np.array_equal(out["Scw"][:12], ref["Scw"]) and np.array_equal(out["chi2"], ref["chi2"])


@pytest.mark.parametrize("case", ["no_edges", "all_fixed"])
def test_nothing_to_optimise(gpu, case):
    pr = dict(ec.ring_case("n12_free"))
    if case == "no_edges":
        for f, dt in (("edge_i", np.int32), ("edge_j", np.int32), ("edge_loop", np.uint8)):
            pr[f] = np.zeros(0, dt)
    else:
        pr["fixed"] = np.ones(12, np.uint8)
    pr["mp_pos"] = np.random.default_rng(0).standard_normal((10, 3)).astype(np.float32)
    pr["mp_ref"] = np.arange(10, dtype=np.int32)
    out = _run(pr, 20)
    assert out["n_solves"] == 0 and out["lm_trials"] == 0 and len(out["chi2"]) == 1
    assert np.array_equal(out["Scw"], pr["Scw"])
    if case == "no_edges":
        assert out["chi2"][0] == 0.0
    else:
        ref = ec.ref_optimize(pr, 0)["chi2"][0]
        assert abs(out["chi2"][0] - ref) <= 1e-12 * ref
    T, X = ec.ref_writeback(pr, out["Scw"])
    assert _ulps(out["mp_pos"], X).max() <= 1


# ---------------------------------------------------------------- 5. write-back
def _ulps(a, b):
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


@pytest.mark.parametrize("name", ["n12_free", "n40_fix"])
def test_write_back(gpu, name):
    pr = dict(ec.ring_case(name))
    N = len(pr["fixed"])
    rng = np.random.default_rng(7)
    pr["mp_pos"] = (12 * rng.standard_normal((1000, 3))).astype(np.float32)
    pr["mp_ref"] = rng.integers(-1, N, 1000).astype(np.int32)
    assert (pr["mp_ref"] == -1).any()
    out = _run(pr, 20)
    T, X = ec.ref_writeback(pr, out["Scw"])
    # [R | t / s] of the returned Scw: R entries within 1 ulp of 1, t / s within 1 ulp
    assert np.abs(out["Tcw"][:, :3, :3] - T[:, :3, :3]).max() <= np.spacing(np.float32(1.0))
    assert _ulps(out["Tcw"][:, :3, 3], T[:, :3, 3]).max() <= 1
    assert np.array_equal(out["Tcw"][:, 3], np.tile(np.float32([0, 0, 0, 1]), (N, 1)))
    keep = pr["mp_ref"] < 0
    assert np.array_equal(out["mp_pos"][keep], pr["mp_pos"][keep])
    u = _ulps(out["mp_pos"][~keep], X[~keep])
    print(name, "map points: max ulp distance", u.max())
    assert u.max() <= 1
    no_points = _run(ec.ring_case(name), 20)   # nMP = 0
    assert no_points["mp_pos"].shape == (0, 3) and np.array_equal(no_points["Scw"], out["Scw"])


# ---------------------------------------------------------------- 6. determinism
def test_two_calls_are_bit_identical(gpu):
    pr = ec.ring_case("n40_free")
    a, b = _run(pr, 20), _run(pr, 20)
    assert np.array_equal(a["Scw"].view(np.uint64), b["Scw"].view(np.uint64))
    assert np.array_equal(a["chi2"].view(np.uint64), b["chi2"].view(np.uint64))
    assert a["lm_trials"] == b["lm_trials"]
