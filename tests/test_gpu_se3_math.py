"""The SE3 arithmetic PoseOptimization and the BA engines share (csrc/ba_math.hpp: se3_exp, se3_mul,
se3_map, quat_from_R / quat_to_R through the float pose conversions), one call each through
orbgpu_unit_se3, against g2o's SE3Quat at 50 digits (pose_mp.py).

Rule, per class and output group (q up to sign; t and mapped points scaled by max(1, |ref|_inf)):
E_gpu <= 8 E_64 + 8 * 2^-52, where E is the largest distance to the 50-digit value over the class
and E_64 is that of the float64 NumPy restatement (rotation matrices) on the same inputs.  The float
pose out of an SE3 is compared entry by entry before the rule (both sides round the same number to
float32, so E is dominated by that rounding).  test_pose_mp_cpu.py shows that the rule fails the
restatement with planted flaws and that no input sits within 1e-6 (relative) of exp's threshold.

exp and the product are also held bit for bit to the oracle inside PoseOptimization
(test_gpu_pose.py); the oracle exports no entry for them alone."""
import numpy as np
import pytest

import pose_mp as pm
import pose_stage_cases as pc
from pose_units import unit_se3

pytestmark = pytest.mark.gpu


def _check(label, E_gpu, E_64, gpu):
    for k in E_64:
        print("%s %-3s E_gpu %.3e  E_64 %.3e  ratio %.2f" % (label, k, E_gpu[k], E_64[k],
                                                             E_gpu[k] / E_64[k] if E_64[k] else (0.0 if E_gpu[k] == 0 else np.inf)))
    assert np.all(np.isfinite(gpu))
    assert pm.within_bound(E_gpu, E_64), (label, E_gpu, E_64)


@pytest.mark.parametrize("name", sorted(pc.exp_inputs()))
def test_exp(gpu, name):
    u = pc.exp_inputs()[name]
    ref, arms = pc.exp_reference(name)
    if name in ("axis_T2.5", "axis_Tpi"):   # rotations about x, y, z beyond 2 pi / 3: the three diagonal arms
        assert set(arms) == {1, 2, 3}
    out = unit_se3("exp", u)
    assert np.all(out[:, 3] >= 0)
    _check("exp " + name, pm.se3_errors(out, ref), pm.se3_errors(pm.f64("exp", u), ref), out)


def test_mul_map(gpu):
    g = pc.group_inputs()
    out = unit_se3("mul", g["a"], g["b"])
    ref = pc.group_reference("mul")
    assert np.all(out[:, 3] >= 0)
    _check("mul", pm.se3_errors(out, ref), pm.se3_errors(pm.f64("mul", g["a"], g["b"]), ref), out)
    out = unit_se3("map", g["a"], g["X"])
    ref = pc.group_reference("map")
    _check("map", pm.group_errors("point", out, ref), pm.group_errors("point", pm.f64("map", g["a"], g["X"]), ref), out)


def test_pose_conversions(gpu):
    T = pc.tcw_inputs()
    ref, arms = pc.tcw_reference()
    assert set(arms) == {0, 1, 2, 3}
    out = unit_se3("from_Tcw", T)
    assert np.all(out[:, 3] >= 0)
    _check("Tcw -> Se3", pm.se3_errors(out, ref), pm.se3_errors(pm.f64("from_Tcw", T), ref), out)
    rows = pc.to_tcw_inputs()
    out = unit_se3("to_Tcw", rows)
    assert np.array_equal(out[:, 12:], np.tile(np.float32([0, 0, 0, 1]), (len(rows), 1)))
    _check("Se3 -> Tcw", pc.tcw_errors(out, pc.to_tcw_reference()),
           pc.tcw_errors(pm.f64("to_Tcw", rows), pc.to_tcw_reference()), out)
    # the float32 of a float64 within a few ulp of the restatement's: the same float, or its neighbour
    # where the two float64 straddle a rounding boundary
    f = pm.f64("to_Tcw", rows)
    ulps = np.abs(out.view(np.int32).astype(np.int64) - f.astype(np.float32).view(np.int32).astype(np.int64))
    print("Se3 -> Tcw: %d of %d entries differ from the restatement's float, by at most %d ulp"
          % ((ulps > 0).sum(), ulps.size, ulps.max()))


def test_unit_entry_validates(gpu):
    from c_orb_slam_amd._lib import ORB_E_INVALID, lib, ptr
    a, out = np.zeros((2, 7)), np.full((2, 7), np.nan)
    a[:, 3] = 1
    L = lib()
    assert L.orbgpu_unit_se3(5, 2, ptr(a), None, ptr(out)) == ORB_E_INVALID
    assert L.orbgpu_unit_se3(-1, 2, ptr(a), None, ptr(out)) == ORB_E_INVALID
    assert L.orbgpu_unit_se3(1, 2, ptr(a), None, ptr(out)) == ORB_E_INVALID   # product without b
    assert L.orbgpu_unit_se3(2, 2, ptr(a), None, ptr(out)) == ORB_E_INVALID   # map without a point
    assert L.orbgpu_unit_se3(0, 2, ptr(a), None, None) == ORB_E_INVALID
    assert L.orbgpu_unit_se3(0, -1, ptr(a), None, ptr(out)) == ORB_E_INVALID
    assert L.orbgpu_unit_se3(1, 0, None, None, None) == 0
    assert L.orbgpu_unit_se3(1, 2, ptr(a), ptr(a), ptr(out)) == 0 and np.array_equal(out, a)
