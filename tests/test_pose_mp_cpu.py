"""What the pose stage tests and the SE3 unit tests rest on, without a GPU: the conditions on the
committed cases (pose_stage_cases.py), the float64 restatement (pose_mp.py) against the 50-digit
reference, and that the rule E <= 8 E_64 + 8 * 2^-52 rejects the restatement with each planted flaw.

E_64 ceilings here are reasoned, not measured: the SE3 operations are a few dozen roundings on
numbers of size <= 1 after scaling (64 * 2^-52); an edge's projection is about ten roundings on pixel
coordinates up to 1241 (1241 * 10 * 2^-53 = 1.4e-12 per error entry, and chi2, rho, J and the terms
scaled by their own size inherit at most a small multiple of it: 1e-11)."""
import numpy as np
import pytest

import oracle_lib
import pose_mp as pm
import pose_stage_cases as pc

mp = pm.mp
SE3_CEIL, EDGE_CEIL = 64 * pm.U52, 1e-11
# cases whose robust edges lie on both sides of Huber's delta^2 (the small frames of the pose cases
# start too far from their optimum to have an edge inside it)
BOTH_SIDES = ("n63", "n64", "n65", "mono", "stereo", "alternating", "robust_mixed", "compaction", "sparse")


def _T0_64(name):
    return pm.f64("from_Tcw", [pc.case(name)[0]["Tcw"].reshape(16)])[0]


def _refs(name, T_row=None):
    T_row = _T0_64(name) if T_row is None else T_row
    ed, _ = pc.edges(name)
    _, fl = pc.case(name)
    act = [k for k in range(len(ed)) if not fl[k] & 1]
    return act, [pm.edge_reference(T_row, ed[k], pc.cam(name)) for k in act], \
        [pm.edge_f64(T_row, ed[k], pc.cam(name)) for k in act]


# ---------------------------------------------------------------- the cases' conditions
def test_case_shapes():
    for n, name in zip(pc.COUNTS, pc.COUNT_CASES):
        pr, fl = pc.case(name)
        assert int(pr["has_mp"].sum()) == n == len(fl) and not (fl & 1).any()
    pr, fl = pc.case("compaction")
    assert len(fl) == 130 and int((fl & 1 == 0).sum()) == 65 and (fl[1::2] & 1).all()
    pr, fl = pc.case("sparse")
    kp = np.flatnonzero(pr["has_mp"])
    assert 3 <= len(kp) < 90 and (np.diff(kp) > 1).any()
    assert max(int(pc.case(c)[0]["has_mp"].sum()) for c in pc.MP_CASES) <= 130
    st = {c: np.array([e.stereo for e in pc.edges(c)[0]]) for c in ("mono", "stereo", "alternating", "n65")}
    assert not st["mono"].any() and st["stereo"].all() and st["n65"].any() and not st["n65"].all()
    assert st["alternating"][0::2].all() and not st["alternating"][1::2].any()
    assert not (pc.case("no_robust")[1] & 2).any()
    f = pc.case("robust_mixed")[1]
    assert (f & 2).any() and not (f & 2).all()


def test_pose_cases_hit_every_quaternion_arm():
    for name, arm in pc.ARMS.items():
        T = pc.case(name)[0]["Tcw"]
        assert pm.from_Tcw(T)[1] == arm, name
    R = pc.case("float_R")[0]["Tcw"][:3, :3].astype(np.float64)
    assert np.abs(R @ R.T - np.eye(3)).max() > 0          # the float rounding of a rotation
    assert np.array_equal(pc.case("identity")[0]["Tcw"], np.eye(4, dtype=np.float32))
    assert set(pc.tcw_reference()[1]) == {0, 1, 2, 3}


@pytest.mark.parametrize("name", pc.MP_CASES)
def test_edges_keep_clear_of_thresholds(name):
    """no chi2 within 1e-6 (relative) of Huber's delta^2, no stereo 1 / p_z within 2^-40 (relative) of
    a float32 rounding midpoint, every point in front of the camera: zero edges excluded"""
    act, refs, _ = _refs(name)
    assert len(act) >= 3
    assert min(float(r["delta_margin"]) for r in refs) >= 1e-6
    mz = [float(r["invz_margin"]) for r in refs if "invz_margin" in r]
    assert not mz or min(mz) >= 2.0 ** -40
    assert all(r["pz"] > 1 for r in refs)
    ed, _ = pc.edges(name)
    if name in BOTH_SIDES:                                  # both sides of delta^2 among the robust edges
        side = [r["chi2"] > pm._f(ed[k].delta) ** 2 for k, r in zip(act, refs) if ed[k].robust]
        assert any(side) and not all(side), name


def test_exp_inputs_keep_clear_of_the_threshold():
    for name, u in pc.exp_inputs().items():
        th = [mp.sqrt(sum(mp.mpf(float(v)) ** 2 for v in r[:3])) for r in u]
        assert min(float(pm.threshold_margin(t)) for t in th) >= 1e-6, name
        assert np.abs(u[:, 3:]).max() <= 10.0 + 1e-9
    below = pc.exp_inputs()["Tbelow"]
    assert all(mp.sqrt(sum(mp.mpf(float(v)) ** 2 for v in r[:3])) < pm.EPS for r in below)
    assert set(pc.exp_reference("axis_T2.5")[1]) == set(pc.exp_reference("axis_Tpi")[1]) == {1, 2, 3}
    assert set(pc.exp_reference("axis_T0.1")[1]) == {0}


# ---------------------------------------------------------------- the restatement against 50 digits
def _se3_E64():
    g = pc.group_inputs()
    E = {}
    for name, u in pc.exp_inputs().items():
        E["exp " + name] = pm.se3_errors(pm.f64("exp", u), pc.exp_reference(name)[0])
    E["mul"] = pm.se3_errors(pm.f64("mul", g["a"], g["b"]), pc.group_reference("mul"))
    E["map"] = pm.group_errors("point", pm.f64("map", g["a"], g["X"]), pc.group_reference("map"))
    E["from_Tcw"] = pm.se3_errors(pm.f64("from_Tcw", pc.tcw_inputs()), pc.tcw_reference()[0])
    return E


def test_se3_restatement_is_ulp_close():
    for label, E in _se3_E64().items():
        print(label, {k: "%.3e" % v for k, v in E.items()})
        # g2o's general arm forms (1 - cos theta) / theta^2 with a relative error of 2^-53 / (theta^2 / 2):
        # V's term of size theta |upsilon| / 2 carries it into t as 2^-53 |upsilon| / theta (|upsilon| <= 10)
        th = pc.THETA.get(label[4:].replace("axis_", ""), 1.0) if label.startswith("exp ") else 1.0
        ceil_t = SE3_CEIL + (2.0 ** -53 * 10 / th if th >= 1e-5 else 0.0)
        assert E.get("q", 0) <= SE3_CEIL and E.get("t", 0) <= ceil_t and E.get("x", 0) <= SE3_CEIL, (label, E)
    # the float pose: each entry is the float32 rounding of a number within SE3_CEIL of the reference
    E = pc.tcw_errors(pm.f64("to_Tcw", pc.to_tcw_inputs()), pc.to_tcw_reference())
    print("to_Tcw", E)
    assert E["R"] <= 2.0 ** -24 + SE3_CEIL and E["t"] <= 2.0 ** -24 + SE3_CEIL


@pytest.mark.parametrize("name", pc.MP_CASES)
def test_edge_restatement_is_ulp_close(name):
    act, refs, f = _refs(name)
    E = pm.edge_errors(f, refs)
    print(name, {k: "%.3e" % v for k, v in E.items()})
    assert all(v <= EDGE_CEIL for v in E.values()), E
    assert all(o["J"][12:].tolist() == [0.0] * 6 for o, r in zip(f, refs) if "invz_margin" not in r)
    # the terms in the kernel's operation order, from the restatement's J, err and chi2
    ed, _ = pc.edges(name)
    kt = pm.terms_in_kernel_order([o["J"] for o in f], [o["err"] for o in f], [o["chi2"] for o in f],
                                  [ed[k].info for k in act], [ed[k].delta for k in act], [ed[k].robust for k in act])
    k_terms = [dict(terms=t) for t in kt]
    kc = pm.chi2_in_kernel_order([o["err"] for o in f], [ed[k].info for k in act], [ed[k].stereo for k in act])
    assert pm.within_bound(pm.edge_errors([dict(chi2=c) for c in kc], refs, keys=("chi2",)), dict(chi2=E["chi2"]))
    Ek = pm.edge_errors(k_terms, refs, keys=("terms",))
    print(name, "terms in kernel order %.3e" % Ek["terms"])
    assert pm.within_bound(Ek, dict(terms=E["terms"]))


def test_trial_restatement_is_ulp_close():
    rng = np.random.default_rng(5)
    T = _T0_64("rot179y")
    for scale in (1e-7, 1e-3, 0.3):
        x = rng.standard_normal(6) * scale
        ref = pm.to_row(pm.mul(pm.exp(x), pm.from_row(T)))
        E = pm.se3_errors([pm.trial64(x, T)], [ref])
        assert all(v <= SE3_CEIL for v in E.values()), (scale, E)


# ---------------------------------------------------------------- the rule rejects every planted flaw
def _edge_flaw_seen(flaw, cases):
    seen = []
    for name in cases:
        act, refs, clean = _refs(name)
        with pm.flawed(flaw):
            bad = [pm.edge_f64(_T0_64(name), pc.edges(name)[0][k], pc.cam(name)) for k in act]
        E64, Ef = pm.edge_errors(clean, refs), pm.edge_errors(bad, refs)
        if not pm.within_bound(Ef, E64):
            seen.append((name, {k: Ef[k] for k in Ef if Ef[k] > 8 * E64[k] + 8 * pm.U52}))
    return seen


@pytest.mark.parametrize("flaw", pm.FLAWS)
def test_flaw_is_rejected(flaw):
    if flaw in ("exp_eps_1e-4", "V_theta2"):
        seen = []
        for name, u in pc.exp_inputs().items():
            ref = pc.exp_reference(name)[0]
            E64 = pm.se3_errors(pm.f64("exp", u), ref)
            with pm.flawed(flaw):
                Ef = pm.se3_errors(pm.f64("exp", u), ref)
            if not pm.within_bound(Ef, E64):
                seen.append(name)
        print(flaw, "rejected on", seen)
        # a threshold of 1e-4 sends both classes between the two thresholds down the truncated arm
        assert seen and (flaw != "exp_eps_1e-4" or seen == ["Tabove", "T8e-5"])
        return
    seen = _edge_flaw_seen(flaw, ("n65", "stereo", "mono", "no_robust"))
    print(flaw, "rejected on", seen)
    names = [s[0] for s in seen]
    assert names
    if flaw == "bf_row3_missing":
        assert "mono" not in names and all("J" in s[1] for s in seen)
    if flaw == "J_rot_col_sign":
        assert all("J" in s[1] for s in seen)
    if flaw == "huber_weight_squared":      # seen in the terms alone, and only where a robust kernel acts
        assert "no_robust" not in names and all(set(s[1]) == {"terms"} for s in seen)


# ---------------------------------------------------------------- the oracle starts from the reference's chi2
def test_oracle_trace_starts_from_the_reference_chi2():
    pr, fl = pc.case("n9")
    assert (fl == 2).all()                                 # round 1 of PoseOptimization: all active and robust
    o = oracle_lib.oracle_pose_optimization(pr)
    act, refs, f = _refs("n9", [float(v) for v in pm.from_Tcw(pr["Tcw"])[0]])
    ref = sum(r["rho"] for r in refs)
    E_o = dict(chi2=float(abs(pm._f(o["solve_ini_chi2"][0]) - ref) / max(1, ref)))
    E_64 = dict(chi2=float(abs(pm._f(sum(x["rho"] for x in f)) - ref) / max(1, ref)))
    print("oracle's first chi2 %.17g, reference %s: E_oracle %.3e, E_64 %.3e"
          % (o["solve_ini_chi2"][0], mp.nstr(ref, 20), E_o["chi2"], E_64["chi2"]))
    assert pm.within_bound(E_o, E_64)
