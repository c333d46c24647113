"""The Sim3 arithmetic the Sim3 engines share (csrc/sim3_math.hpp: exp, log, product, inverse, map)
and EdgeSim3's error, one call each through orbgpu_unit_sim3, against g2o's formulas at 50 digits
(sim3_mp.py).

Rule, per class and output group (q up to sign; t, upsilon and mapped points scaled by
max(1, |ref|_inf); s relative; omega and sigma absolute): E_gpu <= 8 E_64 + 8 * 2^-52, where E is
the largest distance to the 50-digit value over the class and E_64 is that of the float64 NumPy
restatement (essgraph_cases, rotation matrices) on the same inputs.  Both evaluate g2o's
cancelling formulas, which near the thresholds lose many digits on either path alike; the factor 8
is for the different association (quaternions on the device, matrices in NumPy).
test_sim3_mp_cpu.py shows that the rule fails the restatement against deliberately altered
references and that no input sits within 1e-6 (relative) of a branch threshold.

exp, product and inverse are also held bit for bit to the oracle inside OptimizeSim3
(test_gpu_sim3opt.py); the oracle exports no entry for them alone."""
import numpy as np
import pytest

import sim3_mp as sm
from essgraph_units import unit_sim3

pytestmark = pytest.mark.gpu


def _check(label, kind, gpu, f64, ref):
    E_gpu, E_64 = sm.group_errors(kind, gpu, ref), sm.group_errors(kind, f64, ref)
    for k in E_64:
        print("%s %-8s E_gpu %.3e  E_64 %.3e  ratio %.2f" % (label, k, E_gpu[k], E_64[k],
                                                             E_gpu[k] / E_64[k] if E_64[k] else np.inf))
    assert np.all(np.isfinite(gpu))
    assert sm.within_bound(E_gpu, E_64), (label, E_gpu, E_64)


@pytest.mark.parametrize("name", sorted(sm.exp_inputs()))
def test_exp(gpu, name):
    u = sm.exp_inputs()[name]
    ref, arms = sm.exp_reference(name)
    if name in ("axis_T2.5", "axis_Tpi"):   # rotations about x, y, z beyond 2 pi / 3: the three diagonal arms
        assert set(arms) == {1, 2, 3}
    elif name.startswith("axis_"):
        assert set(arms) == {0}
    _check("exp " + name, "sim3", unit_sim3("exp", u), sm.f64("exp", u), ref)


@pytest.mark.parametrize("name", sorted(sm.exp_inputs()))
def test_log(gpu, name):
    rows = sm.log_inputs()[name]
    _check("log " + name, "log", unit_sim3("log", rows), sm.f64("log", rows), sm.log_reference(name))


def test_mul_inverse_map(gpu):
    g = sm.group_inputs()
    _check("mul", "sim3", unit_sim3("mul", g["a"], g["b"]), sm.f64("mul", g["a"], g["b"]), sm.group_reference("mul"))
    _check("inverse", "sim3", unit_sim3("inverse", g["a"]), sm.f64("inverse", g["a"]), sm.group_reference("inverse"))
    _check("map", "point", unit_sim3("map", g["a"], g["X"]), sm.f64("map", g["a"], g["X"]), sm.group_reference("map"))


def test_edge_error(gpu):
    M, Si, Sj = sm.edge_error_inputs()
    _check("edge error", "log", unit_sim3("edge_error", M, Si, Sj), sm.f64("edge_error", M, Si, Sj),
           sm.edge_error_reference())


def test_unit_entry_validates(gpu):
    from c_orb_slam_amd._lib import ORB_E_INVALID, lib, ptr
    a, out = np.zeros((2, 8)), np.zeros((2, 8))
    a[:, 3] = a[:, 7] = 1
    L = lib()
    assert L.orbgpu_unit_sim3(6, 2, ptr(a), None, None, ptr(out)) == ORB_E_INVALID
    assert L.orbgpu_unit_sim3(2, 2, ptr(a), None, None, ptr(out)) == ORB_E_INVALID   # mul without b
    assert L.orbgpu_unit_sim3(5, 2, ptr(a), ptr(a), None, ptr(out)) == ORB_E_INVALID
    assert L.orbgpu_unit_sim3(3, 0, None, None, None, None) == 0
    assert L.orbgpu_unit_sim3(3, 2, ptr(a), None, None, ptr(out)) == 0 and np.array_equal(out, a)
