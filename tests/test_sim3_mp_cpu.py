"""The 50-digit Sim3 reference (sim3_mp.py) without a GPU: that it is right, that the input batches
of test_gpu_sim3_math.py and the graphs of test_gpu_essgraph_stages.py stay clear of g2o's branch
thresholds (so the device, NumPy and mpmath cannot take different arms over a last-ulp
difference), and that the bounds of those tests discriminate: the float64 NumPy restatement, held
to a deliberately altered reference by the same rule, fails."""
import mpmath as mp
import numpy as np
import pytest

import essgraph_cases as ec
import sim3_mp as sm

GENERAL = ("T0.1_Sabove", "T0.1_S0.1", "T1_S0.1", "T2.5_S0.1", "Tpi_S0.1", "T1_S1e-3", "T1_S1")


# ---------------------------------------------------------------- the reference is right
@pytest.mark.parametrize("name", GENERAL)
def test_exp_equals_expm_of_the_generator(name):
    worst = mp.mpf(0)
    for u in sm.exp_inputs()[name][:24]:
        R, t, s = sm.exp(u)
        G = sm.exp_generator(u)
        worst = max([worst] + [abs(G[i, j] - s * R[i][j]) for i in range(3) for j in range(3)]
                    + [abs(G[i, 3] - t[i]) / max(1, abs(t[i])) for i in range(3)])
    assert worst <= mp.mpf("1e-30")


@pytest.mark.parametrize("name", GENERAL)
def test_log_inverts_exp_in_the_general_branch(name):
    worst = mp.mpf(0)
    for u in sm.exp_inputs()[name][:24]:
        S = sm.exp(u)
        assert sm.log_d(S) < 1 - sm.EPS and abs(mp.mpf(float(u[6]))) > sm.EPS
        worst = max([worst] + [abs(a - mp.mpf(float(b))) / max(1, abs(b)) for a, b in zip(sm.log(S), u)])
    assert worst <= mp.mpf("1e-30")


def test_quaternion_round_trip():
    """from_row(to_row(S)) gives S back, in each of the four matrix -> quaternion arms"""
    seen = set()
    for name in ("T1_S0.1", "axis_T2.5", "axis_Tpi"):
        for u in sm.exp_inputs()[name][:12]:
            S = sm.exp(u)
            q, arm = sm.quat_from_R(S[0])
            seen.add(arm)
            R2 = sm.from_row(q + [0, 0, 0, 1])[0]
            assert max(abs(R2[i][j] - S[0][i][j]) for i in range(3) for j in range(3)) <= mp.mpf("1e-40")
    assert seen == {0, 1, 2, 3}


# ---------------------------------------------------------------- input conditions
def _theta(u):
    return mp.sqrt(sum(mp.mpf(float(x)) ** 2 for x in u[:3]))


@pytest.mark.parametrize("name", sorted(sm.exp_inputs()))
def test_exp_and_log_batches_are_clear_of_the_thresholds(name):
    u = sm.exp_inputs()[name]
    assert len(u) % 256 != 0 and len(u) > 256
    for row in u:
        assert sm.threshold_margin(_theta(row)) >= 1e-6 and sm.threshold_margin(abs(mp.mpf(float(row[6])))) >= 1e-6
    for row in sm.log_inputs()[name]:
        S = sm.from_row(row)
        assert sm.threshold_margin(1 - sm.log_d(S)) >= 1e-6
        assert sm.threshold_margin(abs(mp.log(S[2]))) >= 1e-6
        assert sm.log_d(S) > -1 + mp.mpf("1e-5")   # theta <= pi - 0.01: d = -1 is never evaluated


def test_threshold_classes_sit_where_they_claim():
    """'just below' and 'just above' are factors of 1 -+ 1e-3 of each threshold, on both sides"""
    U = sm.exp_inputs()
    for name, lo, hi in (("Tbelow_Sbelow", True, True), ("Tbelow_Sabove", True, False), ("Tabove_Sbelow", False, True),
                         ("Tabove_Sabove", False, False)):
        for row in U[name]:
            th, sg = _theta(row) / sm.EPS, abs(mp.mpf(float(row[6]))) / sm.EPS
            assert abs(th - (1 - 1e-3 if lo else 1 + 1e-3)) <= 1e-6 and abs(sg - (1 - 1e-3 if hi else 1 + 1e-3)) <= 1e-6
    for name, inside in (("Tlog_in_S0.1", True), ("Tlog_out_S0.1", False), ("Tlog_in_S0", True), ("Tlog_out_S0", False)):
        for row in sm.log_inputs()[name]:
            r = (1 - sm.log_d(sm.from_row(row))) / sm.EPS
            assert abs(r - (1 - 1e-3 if inside else 1 + 1e-3)) <= 1e-6
            assert (sm.log_d(sm.from_row(row)) > 1 - sm.EPS) == inside


def test_every_branch_and_quaternion_arm_is_in_the_batches():
    U = sm.exp_inputs()
    arms = set()
    for name in U:
        if name.startswith("axis_"):
            arms |= set(sm.exp_reference(name)[1])
    assert arms == {0, 1, 2, 3}
    branches = {(bool(_theta(U[n][0]) < sm.EPS), bool(abs(U[n][0][6]) < sm.EPS)) for n in U}
    assert len(branches) == 4
    logb = {(bool(sm.log_d(sm.from_row(r[0])) > 1 - sm.EPS), bool(abs(mp.log(mp.mpf(float(r[0][7])))) < sm.EPS))
            for r in sm.log_inputs().values()}
    assert len(logb) == 4
    g = sm.group_inputs()
    assert g["a"][:, 7].min() < 0.15 and g["a"][:, 7].max() > 7 and np.abs(g["a"][:, 4:7]).max() > 90
    assert np.abs(g["X"]).max() > 900
    assert max(np.linalg.norm(u[:, 3:6], axis=1).max() for u in U.values()) > 90


@pytest.mark.parametrize("name", ["g1_free", "g1_fix"])
def test_g1_edges_are_clear_of_the_thresholds(name):
    """the errors of the G1 graphs (and so their +-1e-9 perturbations, which move d and sigma by
    1e-9) are far from log's thresholds; the perturbations themselves are far below exp's"""
    pr = ec.stage_graph(name)
    M = sm.measurements(pr)
    est = [sm.from_row(r) for r in pr["Scw"]]
    for e in range(len(M)):
        E = sm.mul(sm.mul(M[e], est[pr["edge_i"][e]]), sm.inv(est[pr["edge_j"][e]]))
        assert sm.threshold_margin(1 - sm.log_d(E)) >= 1e-2 and sm.threshold_margin(abs(mp.log(E[2]))) >= 1e-2
    assert sm.threshold_margin(sm.DELTA) >= 0.99


@pytest.mark.parametrize("name", ec.STAGE_GRAPHS)
def test_stage_graphs_have_the_structure_they_claim(name):
    pr = ec.stage_graph(name)
    rows = dict(g1_free=77, g1_fix=77, ring20=140, ring21=147, hub=553, split=168, few_free=35, e1=7, e63=63, e64=35,
                e65=448, big=4102)[name]
    edges = dict(few_free=4097, e1=1, e63=63, e64=64, e65=65).get(name)
    sys_idx, nV = ec.system_index(pr)
    assert 7 * nV == rows and (edges is None or len(pr["edge_i"]) == edges)
    below, above = ec.edge_orders(pr)
    if name != "e1":   # a single edge to a fixed vertex
        assert below >= 1 and above >= 1
    if name == "hub":
        deg = np.bincount(np.concatenate([pr["edge_i"], pr["edge_j"]]), minlength=80)
        pairs = list(zip(pr["edge_i"].tolist(), pr["edge_j"].tolist()))
        assert deg[5] > 64 and len({frozenset(p) for p in pairs}) < len(pairs)
    if name == "split":
        assert pr["fixed"].sum() == 2 and sys_idx[13] == -1 and not pr["fixed"][13]      # the edge-less vertex
        assert sys_idx[12] + 1 == sys_idx[15] and sys_idx[14] == -1                       # the gap it leaves
        touching = (pr["edge_i"] == 20) | (pr["edge_j"] == 20)
        other = np.where(pr["edge_i"] == 20, pr["edge_j"], pr["edge_i"])[touching]
        assert touching.sum() == 3 and pr["fixed"][other].all() and sys_idx[20] >= 0     # edges to fixed vertices only
        first = (pr["edge_i"] < 13) & (pr["edge_j"] < 13)
        second = (pr["edge_i"] > 13) & (pr["edge_j"] > 13)
        free_both = (sys_idx[pr["edge_i"]] >= 0) & (sys_idx[pr["edge_j"]] >= 0)
        assert np.all((first | second)[free_both])                                         # two components


@pytest.mark.parametrize("name", ["g1_free", "g1_fix", "hub", "split"])
def test_end_to_end_graphs_are_well_conditioned(name):
    """the graphs the optimiser is run on end to end: the reference's rounding variants agree far
    inside the tolerances of that comparison, as test_essgraph_cpu.py asserts for the ring cases"""
    pr = ec.stage_graph(name)
    refs = tuple(ec.ref_optimize(pr, 20, v) for v in range(3))
    ini, fin, pose = ec.variant_spread(refs)
    print(name, "spread: initial chi2 %.2e final chi2 %.2e pose %.2e" % (ini, fin, pose))
    assert ini <= 1e-12 and fin <= 1e-7 and pose <= 1e-4
    assert refs[0]["chi2"][-1] < 0.5 * refs[0]["chi2"][0]


# ---------------------------------------------------------------- the tests discriminate
def _fails_against(kind, out64, ref_true, ref_altered):
    E_64 = sm.group_errors(kind, out64, ref_true)
    E_alt = sm.group_errors(kind, out64, ref_altered)
    assert sm.within_bound(E_64, E_64)
    return not sm.within_bound(E_alt, E_64), E_64, E_alt


@pytest.mark.parametrize("flaw,name", [("B_half_small_theta", "T0_S1"), ("B_half_small_theta", "T0_S0.1"),
                                       ("B_half_general", "T1_S0.1"), ("B_half_general", "T1e-3_S0.1"),
                                       ("exp_eps_1e-4", "T8e-5_S0.1"), ("exp_eps_1e-4", "T8e-5_S1e-3"),
                                       ("omega_sign", "T1_S0.1"), ("omega_sign", "T0_S0")])
def test_altered_exp_is_caught(flaw, name):
    u = sm.exp_inputs()[name]
    with sm.flawed(flaw):
        altered = [sm.to_row(sm.exp(row)) for row in u]
    failed, E_64, E_alt = _fails_against("sim3", sm.f64("exp", u), sm.exp_reference(name)[0], altered)
    print(flaw, name, "E_64", E_64, "against the altered reference", E_alt)
    assert failed


@pytest.mark.parametrize("flaw,name", [("B_half_small_theta", "T0_S1"), ("B_half_general", "T1_S0.1")])
def test_altered_log_is_caught(flaw, name):
    rows = sm.log_inputs()[name]
    with sm.flawed(flaw):
        altered = [sm.log(sm.from_row(r)) for r in rows]
    failed, E_64, E_alt = _fails_against("log", sm.f64("log", rows), sm.log_reference(name), altered)
    print(flaw, name, "E_64", E_64, "against the altered reference", E_alt)
    assert failed


@pytest.mark.parametrize("name", ["g1_free", "g1_fix"])
def test_swapped_jacobian_side_is_caught(name):
    """the J rule of the stage tests, max |J - J_mp| <= 8 max |J_64 - J_mp| over the free vertices'
    blocks, with the reference's side index swapped"""
    pr = ec.stage_graph(name)
    M = ec.QuatAlgebra.to_rows(ec.measurements(pr, ec.QuatAlgebra))
    J64 = ec.numeric_jacobian(ec.rows_to_sim3(M), ec.rows_to_sim3(pr["Scw"]), pr["edge_i"], pr["edge_j"],
                              bool(pr["bFixScale"])).transpose(1, 0, 2, 3)
    _, Jmp = sm.linearise(pr, M)
    with sm.flawed("J_side_swap"):
        _, Jalt = sm.linearise(pr, M)
    free = np.stack([~pr["fixed"][pr["edge_i"]].astype(bool), ~pr["fixed"][pr["edge_j"]].astype(bool)], 1)
    noise = np.abs(J64 - Jmp)[free].max()
    both = free.all(1)   # an edge to a fixed vertex has one block: swapping it moves it to the unread side
    wrong = np.abs(J64 - Jalt)[both].max()
    print(name, "J noise of the float64 restatement %.2e, |J| up to %.2f; against the swapped reference %.2e"
          % (noise, np.abs(Jmp).max(), wrong))
    assert noise < 1e-4 and wrong > 8 * noise


def test_flipped_gather_side_is_caught_only_on_a_graph_with_both_edge_directions():
    """The assembly check is bit for bit.  An entry whose side bit is wrong when a < b changes H on
    the flipped graph and changes nothing on the original ring, whose edges all run from the higher
    system index to the lower: the arm was never executed."""
    for name, caught in (("g1_free", True), (None, False)):
        pr = ec.stage_graph(name) if name else ec.ring_case("n12_free")
        below, above = ec.edge_orders(pr)
        assert (below > 0) == caught and above > 0
        M = ec.measurements(pr)
        est = ec.rows_to_sim3(pr["Scw"])
        J = np.ascontiguousarray(ec.numeric_jacobian(M, est, pr["edge_i"], pr["edge_j"], False).transpose(1, 0, 2, 3))
        err = ec.edge_errors(M, ec.take(est, pr["edge_i"]), ec.take(est, pr["edge_j"]), 0)
        sys_idx, nV = ec.system_index(pr)
        H, b = ec.assemble_f64(J, err, pr["edge_i"], pr["edge_j"], sys_idx, nV, 1e-16)
        H2, b2 = ec.assemble_f64(J, err, pr["edge_i"], pr["edge_j"], sys_idx, nV, 1e-16, flip_side_when_a_below_b=True)
        assert np.array_equal(b, b2)
        assert (not np.array_equal(H, H2)) == caught
        # the restatement agrees with the reference optimiser's own H to rounding
        Href = np.zeros_like(H)
        for e in range(len(err)):
            a, c = sys_idx[pr["edge_i"][e]], sys_idx[pr["edge_j"][e]]
            if a >= 0:
                Href[7 * a:7 * a + 7, 7 * a:7 * a + 7] += J[e, 0].T @ J[e, 0]
            if c >= 0:
                Href[7 * c:7 * c + 7, 7 * c:7 * c + 7] += J[e, 1].T @ J[e, 1]
            if a >= 0 and c >= 0:
                lo, hi, Jl, Jh = (a, c, J[e, 0], J[e, 1]) if a < c else (c, a, J[e, 1], J[e, 0])
                Href[7 * lo:7 * lo + 7, 7 * hi:7 * hi + 7] += Jl.T @ Jh
        Href = np.triu(Href) + 1e-16 * np.eye(len(Href))
        assert np.abs(H - Href).max() <= 1e-12 * np.abs(Href).max()


def test_csum_restatement_matches_the_oracle():
    import ctypes as C
    import oracle_lib
    L = oracle_lib.lib()
    L.ora_csum.restype = C.c_double
    L.ora_csum.argtypes = [C.c_void_p, C.c_int]
    rng = np.random.default_rng(5)
    for n in (1, 2, 7, 63, 64, 65, 448, 4096, 4097, 4102, 70000):
        v = rng.standard_normal(n) * 10.0 ** rng.integers(-8, 8, n)
        w = v.copy()
        assert ec.csum(v) == L.ora_csum(w.ctypes.data, n)
    assert np.signbit(ec.csum([-0.0]))
