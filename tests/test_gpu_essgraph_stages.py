"""OptimizeEssentialGraph stage by stage: one linearisation and one LM trial through
orbgpu_unit_essgraph_stage (the engine's own launches), each intermediate held to what defines it.

  measurements, errors, the update   g2o at 50 digits (sim3_mp.py), E_gpu <= 8 E_64 + 8 * 2^-52
  J                                  the exact-arithmetic central differences: within 8 x the
                                     float64 restatement's own distance to them
  H, b                               bit for bit a float64 restatement of k_ess_assemble on the
                                     device's own J and errors, its gather lists built here from
                                     the edge list alone
  x                                  backward error within 8 x LAPACK's on the device's own H, b
  chi2, trial chi2, computeScale     bit for bit ora_csum of the device's own terms

The graphs (essgraph_cases.stage_graph) have edges in both directions of the system order, both
sides of the dense solver's limit (140 and 147 rows), a hub of degree 84, two components, a vertex
joined to fixed vertices only, a gap in sysIdx, and sums of 1, 63, 64, 65, 4,097 and 4,102 terms."""
import functools

import mpmath as mp
import numpy as np
import pytest

import essgraph_cases as ec
import sim3_mp as sm
from essgraph_units import ess_dense_max, stage

pytestmark = pytest.mark.gpu

SOLVER = dict(g1_free=0, g1_fix=0, ring20=0, ring21=1, hub=1, split=1, few_free=0, e1=0, e63=0, e64=0, e65=1, big=1)
LAMBDA0 = 1e-16


@functools.lru_cache(maxsize=None)
def _stage(name, lam_kind="tiny", tiled=False):
    """lam_kind 'tiny': g2o's initial 1e-16; 'mean': 1e-3 of H's mean diagonal.  (do not modify)"""
    pr = ec.stage_graph(name)
    lam = LAMBDA0
    if lam_kind == "mean":
        H0 = _stage(name, "tiny", tiled)["H"]
        lam = 1e-3 * float(np.mean(np.diag(H0)))
    if tiled:
        with ess_dense_max(0):
            out = stage(pr, lam, want_H=name != "big")
    else:
        out = stage(pr, lam, want_H=name != "big")
    out["lambda"] = lam
    return out


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _free_blocks(pr):
    return np.stack([~pr["fixed"][pr["edge_i"]].astype(bool), ~pr["fixed"][pr["edge_j"]].astype(bool)], 1)


# ---------------------------------------------------------------- structure
@pytest.mark.parametrize("name", ec.STAGE_GRAPHS)
def test_system_index_and_solver(gpu, name):
    pr, o = ec.stage_graph(name), _stage(name)
    sys_idx, nV = ec.system_index(pr)
    below, above = ec.edge_orders(pr)
    assert name == "e1" or (below >= 1 and above >= 1)
    assert o["nV"] == nV and np.array_equal(o["sysIdx"], sys_idx)
    print(name, "rows", 7 * nV, "solver", o["solver"])
    assert o["solver"] == SOLVER[name] and o["ok"] == 1


def test_dense_limit_knob(gpu):
    from c_orb_slam_amd._lib import ORB_E_INVALID, lib
    assert lib().orbgpu_unit_set_ess_dense_max(-1) == ORB_E_INVALID
    assert lib().orbgpu_unit_set_ess_dense_max(145) == ORB_E_INVALID
    assert _stage("g1_free", "tiny", True)["solver"] == 1 and _stage("g1_free")["solver"] == 0


# ---------------------------------------------------------------- 1. measurements and errors
@pytest.mark.parametrize("name", ["g1_free", "g1_fix"])
def test_measurements_and_errors(gpu, name):
    pr, o = ec.stage_graph(name), _stage(name)
    ref = [sm.to_row(S) for S in sm.measurements(pr)]
    f64 = sm.R_rows_f64(*ec.measurements(pr))
    E_gpu, E_64 = sm.group_errors("sim3", o["meas"], ref), sm.group_errors("sim3", f64, ref)
    print(name, "meas E_gpu", E_gpu, "E_64", E_64)
    assert sm.within_bound(E_gpu, E_64)
    M = o["meas"]   # the errors of the device's own measurements
    est = [sm.from_row(r) for r in pr["Scw"]]
    ref = [sm.edge_error(sm.from_row(M[e]), est[pr["edge_i"][e]], est[pr["edge_j"][e]]) for e in range(len(M))]
    f64 = sm.f64("edge_error", M, pr["Scw"][pr["edge_i"]], pr["Scw"][pr["edge_j"]])
    E_gpu, E_64 = sm.group_errors("log", o["err"], ref), sm.group_errors("log", f64, ref)
    print(name, "err E_gpu", E_gpu, "E_64", E_64)
    assert sm.within_bound(E_gpu, E_64)


@pytest.mark.parametrize("name", ec.STAGE_GRAPHS)
def test_edge_chi2_is_the_sequential_sum_of_squares(gpu, name):
    o = _stage(name)
    c = np.zeros(len(o["err"]))
    for k in range(7):
        c = c + o["err"][:, k] * o["err"][:, k]
    assert np.array_equal(_bits(o["chi2e"]), _bits(c))
    assert np.all(np.isfinite(o["chi2e_trial"]))


# ---------------------------------------------------------------- 2. J
@pytest.mark.parametrize("name", ["g1_free", "g1_fix"])
def test_jacobian_against_exact_central_differences(gpu, name):
    pr, o = ec.stage_graph(name), _stage(name)
    fix = bool(pr["bFixScale"])
    _, Jmp = sm.linearise(pr, o["meas"])
    J64 = ec.numeric_jacobian(ec.rows_to_sim3(o["meas"]), ec.rows_to_sim3(pr["Scw"]), pr["edge_i"], pr["edge_j"],
                              fix).transpose(1, 0, 2, 3)
    free = _free_blocks(pr)
    noise = np.abs(J64 - Jmp)[free].max()
    err = np.abs(o["J"] - Jmp)[free].max()
    print("%s: |J| up to %.2f; float64 restatement's J noise %.3e; device's J error %.3e (ratio %.2f)"
          % (name, np.abs(Jmp).max(), noise, err, err / noise))
    assert err <= 8 * noise
    if fix:
        assert np.array_equal(_bits(o["J"][free][:, :, 6]), _bits(np.zeros_like(o["J"][free][:, :, 6])))
        assert np.all(Jmp[free][:, :, 6] == 0)


# ---------------------------------------------------------------- 3. assembly
# every graph at both lambdas (the 4,102-row graph, whose H is not fetched, at the first alone: b
# only), and G1 through the tiles
ASSEMBLY = ([(g, k, False) for g in ec.STAGE_GRAPHS for k in ("tiny", "mean") if (g, k) != ("big", "mean")]
            + [("g1_free", "tiny", True), ("g1_free", "mean", True), ("g1_fix", "mean", True)])


@pytest.mark.parametrize("name,lam_kind,tiled", ASSEMBLY)
def test_assembly_is_bit_exact(gpu, name, lam_kind, tiled):
    pr, o = ec.stage_graph(name), _stage(name, lam_kind, tiled)
    H, b = ec.assemble_f64(o["J"], o["err"], pr["edge_i"], pr["edge_j"], o["sysIdx"], o["nV"], o["lambda"],
                           want_H=o["H"] is not None)
    assert np.array_equal(_bits(o["b"]), _bits(b))
    if o["H"] is not None:
        assert np.array_equal(_bits(o["H"]), _bits(H)), np.argwhere(o["H"] != H)[:5]
    if pr["bFixScale"]:
        s = np.arange(6, o["n"], 7)
        Hs = o["H"] + np.triu(o["H"], 1).T
        assert np.all(o["H"][s, s] == o["lambda"]) and np.all(o["b"][s] == 0)
        Hs[s, s] = 0
        assert np.all(Hs[s] == 0)


# ---------------------------------------------------------------- 4. the solve
def _eta(H, x, b):
    L = np.longdouble
    Hs = (H + np.triu(H, 1).T).astype(L)
    r = np.abs(Hs @ x.astype(L) - b.astype(L)).max()
    return float(r / (np.abs(Hs).sum(1).max() * np.abs(x).max() + np.abs(b).max()))


@pytest.mark.parametrize("lam_kind", ["tiny", "mean"])
@pytest.mark.parametrize("name,tiled", [("g1_free", False), ("g1_fix", False), ("ring20", False), ("ring21", False),
                                        ("hub", False), ("split", False), ("g1_free", True), ("e65", False)])
def test_solve_backward_error(gpu, name, tiled, lam_kind):
    o = _stage(name, lam_kind, tiled)
    H, b, x, n = o["H"], o["b"], o["x_solve"], o["n"]
    x_lapack = np.linalg.solve(H + np.triu(H, 1).T, b)
    eta, eta_lapack = _eta(H, x, b), _eta(H, x_lapack, b)
    print("%s%s lambda %.3e: %d rows, solver %d, eta %.3e, eta_lapack %.3e"
          % (name, " (dense limit 0)" if tiled else "", o["lambda"], n, o["solver"], eta, eta_lapack))
    assert o["ok"] == 1 and o["solver"] == (1 if tiled else SOLVER[name])
    assert eta <= max(8 * eta_lapack, n * 2.0 ** -53)


# ---------------------------------------------------------------- 5. sums
@pytest.mark.parametrize("name,tiled", [(g, False) for g in ec.STAGE_GRAPHS] + [("g1_free", True)])
def test_sums_are_canonical(gpu, name, tiled):
    for lam_kind in ("tiny",) if name == "big" else ("tiny", "mean"):
        o = _stage(name, lam_kind, tiled)
        x, b, lam = o["x"], o["b"], o["lambda"]
        assert o["chi2"] == ec.csum(o["chi2e"]) and o["chi2_trial"] == ec.csum(o["chi2e_trial"])
        assert o["scale"] == ec.csum(x * (lam * x + b))
    terms = dict(e1=(1, 7), e63=(63, 63), e64=(64, 35), e65=(65, 448), few_free=(4097, 35), big=(1755, 4102))
    if name in terms:
        assert (len(o["chi2e"]), o["n"]) == terms[name]


# ---------------------------------------------------------------- 6. the update
@pytest.mark.parametrize("name", ["g1_free", "g1_fix", "split"])
def test_update(gpu, name):
    pr, o = ec.stage_graph(name), _stage(name, "mean")
    sys_idx, x = o["sysIdx"], o["x"].reshape(-1, 7)
    inside = sys_idx >= 0
    if pr["bFixScale"]:
        assert np.all(x[:, 6] == 0) and np.array_equal(_bits(x[:, :6]), _bits(o["x_solve"].reshape(-1, 7)[:, :6]))
    else:
        assert np.array_equal(_bits(o["x"]), _bits(o["x_solve"]))
    assert np.array_equal(_bits(o["est_trial"][~inside]), _bits(pr["Scw"][~inside]))
    assert (~inside).sum() >= (3 if name == "split" else 1)
    for u in x:   # the device's step must not sit on one of exp's thresholds
        theta = mp.sqrt(sum(mp.mpf(float(v)) ** 2 for v in u[:3]))
        assert sm.threshold_margin(theta) >= 1e-6 and sm.threshold_margin(abs(mp.mpf(float(u[6])))) >= 1e-6
    rows = pr["Scw"][inside][np.argsort(sys_idx[inside])]
    ref = [sm.to_row(sm.mul(sm.exp(u), sm.from_row(r))) for u, r in zip(x, rows)]
    f64 = sm.R_rows_f64(*ec.mul(ec.s3_exp(x), ec.rows_to_sim3(rows)))
    gpu_rows = o["est_trial"][inside][np.argsort(sys_idx[inside])]
    E_gpu, E_64 = sm.group_errors("sim3", gpu_rows, ref), sm.group_errors("sim3", f64, ref)
    print(name, "update E_gpu", E_gpu, "E_64", E_64)
    assert sm.within_bound(E_gpu, E_64)
    assert np.abs(x).max() > 1e-3   # a real step


# ---------------------------------------------------------------- 7. end to end on the new structures
@pytest.mark.parametrize("name,tiled", [("g1_free", False), ("g1_fix", False), ("hub", False), ("split", False),
                                        ("g1_free", True), ("g1_fix", True)])
def test_optimiser_on_the_new_structures(gpu, name, tiled):
    from test_gpu_essgraph import _check_against_reference
    pr = ec.stage_graph(name)
    if tiled:
        with ess_dense_max(0):
            out = _check_against_reference(pr)
    else:
        out = _check_against_reference(pr)
    assert out["n_solves"] >= 1
    if name == "split":   # the edge-less vertex and the fixed ones come back untouched
        keep = ec.system_index(pr)[0] < 0
        assert keep.sum() == 3 and np.array_equal(_bits(out["Scw"][keep]), _bits(pr["Scw"][keep]))


def test_optimiser_just_above_the_dense_limit(gpu):
    pr = ec.stage_graph("ring21")
    assert _stage("ring21")["solver"] == 1 and _stage("ring20")["solver"] == 0
    out = gpu.OptimizeEssentialGraph(pr, 20)
    assert out["n_solves"] >= 1 and out["chi2"][-1] < out["chi2"][0]
