"""CPU: the scalar restatement of LocalMapping::CreateNewMapPoints and the MapPoint updates
(tests/localmap_ref.py, the thing the GPU is compared with bit for bit) against float64
references, and the argument validation of the two C entries."""
import ctypes as C

import numpy as np
import pytest

import c_orb_slam_amd as orb
import localmap_cases as lc
import localmap_ref as lr
from c_orb_slam_amd._lib import (ORB_E_INVALID, ORB_E_NODEVICE, lib, orb_pointupdate, orb_triangulate, ptr)

SCENES = [(kind, frac) for kind in ("sideways", "forward") for frac in (0.0, 0.5, 1.0)]


def _pair_inputs(s, i1, i2):
    """The float32 inputs of one pair as a flat float32 vector (see _ref64_from)."""
    K1, K2 = s["KF1"], s["KF2"]
    k1, k2 = K1.keysUn[i1], K2.keysUn[i2]
    ur1 = K1.uRight[i1] if K1.uRight is not None else -1
    ur2 = K2.uRight[i2] if K2.uRight is not None else -1
    d1 = s["depth1"][i1] if s["depth1"] is not None else -1
    d2 = s["depth2"][i2] if s["depth2"] is not None else -1
    v = [k1["x"], k1["y"], ur1, d1, k2["x"], k2["y"], ur2, d2]
    v += list(K1.Tcw.ravel()[:12]) + list(K2.Tcw.ravel()[:12])
    v += [K1.fx, K1.fy, K1.cx, K1.cy, K2.fx, K2.fy, K2.cx, K2.cy]
    return np.array(v, np.float32), (int(k1["octave"]), int(k2["octave"]))


def _ref64_from(v, octs, s):
    v = v.astype(np.float64)
    T1, T2 = np.eye(4), np.eye(4)
    T1[:3], T2[:3] = v[8:20].reshape(3, 4), v[20:32].reshape(3, 4)
    K1, K2 = s["KF1"], s["KF2"]
    cam1 = tuple(v[32:36]) + (float(K1.bf), float(K1.b))
    cam2 = tuple(v[36:40]) + (float(K2.bf), float(K2.b))
    sf = K1.scale.astype(np.float64)
    sig = s["sigma2"].astype(np.float64)
    return lr.ref64_pair(T1, T2, cam1, cam2, (v[0], v[1], v[2], v[3], octs[0]), (v[4], v[5], v[6], v[7], octs[1]),
                         sf, sf, sig, sig, float(s["scaleFactor"]))


def _ulp_moved(v, rng):
    sign = np.where(rng.random(len(v)) < 0.5, -np.inf, np.inf).astype(np.float32)
    out = np.nextafter(v, sign)
    for j in (2, 6):                      # a monocular keypoint's uRight = -1 is a flag, not a measurement
        if v[j] < 0:
            out[j] = v[j]
    return out


def test_restatement_against_float64_reference():
    """Statuses agree on every pair the float64 reference does not find borderline, and every
    created point lies within 16 x the displacement the float64 reference itself shows when
    each of its float32 inputs moves by one ulp (maximum over 8 random sign patterns).

    Observed with these generators (600 pairs per scene): kept pairs per scene
    600 / 594 / 590 (sideways, stereo fraction 0 / 0.5 / 1) and 599 / 515 / 465 (forward); status
    counts over the kept pairs {1: 1500, 2: 223, 3: 57, 0: 1142, -2/-4: 188, -3/-5: 194, -7: 59};
    worst x3D error / one-ulp displacement 1.04 (the bound is 16)."""
    rng = np.random.default_rng(11)
    counts, kept_per_scene, worst = {}, [], 0.0
    for kind, frac in SCENES:
        s = lc.scene(kind, frac, 600)
        (x3D, status, _, _, _), = lr.restate_batch(s["KF1"], s["depth1"], s["sigma2"], s["scaleFactor"],
                                                   lc.neighbours_of(s))
        kept = 0
        for i, (i1, i2) in enumerate(s["pairs"]):
            v, octs = _pair_inputs(s, i1, i2)
            st, X, border = _ref64_from(v, octs, s)
            if border:
                continue
            kept += 1
            assert status[i] == st, (kind, frac, i, int(status[i]), st)
            counts[st] = counts.get(st, 0) + 1
            if st <= 0:
                continue
            disp = 0.0
            for _ in range(8):
                st2, X2, _ = _ref64_from(_ulp_moved(v, rng), octs, s)
                if st2 == st:
                    disp = max(disp, float(np.linalg.norm(X2 - X)))
            err = float(np.linalg.norm(x3D[i].astype(np.float64) - X))
            assert disp > 0
            worst = max(worst, err / disp)
            assert err <= 16 * disp, (kind, frac, i, st, err, disp)
        kept_per_scene.append(kept)
    merged = {1: counts.get(1, 0), 2: counts.get(2, 0), 3: counts.get(3, 0), 0: counts.get(0, 0),
              "z": counts.get(-2, 0) + counts.get(-4, 0), "reproj": counts.get(-3, 0) + counts.get(-5, 0),
              -7: counts.get(-7, 0)}
    print("kept", kept_per_scene, "status counts", merged, "worst x3D ratio", worst)
    # the generator must keep reaching every branch
    assert min(kept_per_scene) >= 400, kept_per_scene
    for key, cnt in merged.items():
        assert cnt >= 8, (key, merged)


def test_restated_normal_and_depth_of_new_points():
    """The optional outputs of a created point are UpdateNormalAndDepth with observations
    {KF1, KF2} and reference keyframe KF1: the restated pair equals the restated point update."""
    s = lc.scene("sideways", 0.5, 65)
    K1 = lr.KF(s["KF1"], s["depth1"], s["sigma2"])
    K2 = lr.KF(s["KF2"], s["depth2"], s["sigma2"])
    n = 0
    for i1, i2 in s["pairs"]:
        st, X, normal, mx, mn = lr.restate_pair(K1, K2, int(i1), int(i2), float(s["scaleFactor"]))
        if st <= 0:
            continue
        O1, O2 = K1.Twc[3::4], K2.Twc[3::4]
        nr, a, b = lr.restate_normal_depth(X, [O1, O2], O1, K1.sf[K1.oct[i1]], K1.sf[-1])
        assert (nr, a, b) == (normal, mx, mn)
        n += 1
    assert n >= 10


def test_descriptor_choice_median_and_ties():
    """The counting select of the device kernel equals the reference's sort-and-index loop."""
    ties = lc.tie_descriptors()
    assert lr.brute_best(ties["k1"]) == lr.restate_best(ties["k1"]) == 0
    assert lr.brute_best(ties["k2"]) == lr.restate_best(ties["k2"]) == 0
    assert lr.brute_best(ties["all_equal"]) == lr.restate_best(ties["all_equal"]) == 0
    assert lr.brute_best(ties["tie3"]) == lr.restate_best(ties["tie3"]) == 0
    assert lr.brute_best(ties["tie_pair"]) == lr.restate_best(ties["tie_pair"]) == 1
    assert lr.brute_best(ties["far3"]) == lr.restate_best(ties["far3"]) == 1
    assert lr.brute_best(np.zeros((0, 32), np.uint8)) == lr.restate_best(np.zeros((0, 32), np.uint8)) == -1
    ks = [1, 2, 3, 4, 5, 8, 17, 33, 63, 64, 65, 130]
    c = lc.update_case(ks)
    st = c["obs_start"]
    nonzero = 0
    for p in range(len(ks)):
        d = c["obs_desc"][st[p]:st[p + 1]]
        b = lr.brute_best(d)
        assert lr.restate_best(d) == b, ks[p]
        nonzero += b != 0
    assert nonzero >= 3          # the winner is not always the first row


def test_restated_normal_depth_against_float64():
    c = lc.update_case([1, 2, 3, 9, 60])
    st = c["obs_start"]
    for p in range(5):
        args = (c["pos"][p], c["obs_Ow"][st[p]:st[p + 1]], c["ref_Ow"][p], c["ref_scale"][p], c["ref_scale_top"][p])
        n32, mx32, mn32 = lr.restate_normal_depth(*args)
        n64, mx64, mn64 = lr.ref64_normal_depth(*args)
        # a few float32 roundings per observation on values of magnitude <= 1 (normal) or the distance
        k = st[p + 1] - st[p]
        assert np.abs(np.array(n32) - n64).max() <= (k + 3) * 2.0 ** -24
        assert abs(mx32 - mx64) <= 4 * 2.0 ** -24 * mx64 and abs(mn32 - mn64) <= 6 * 2.0 ** -24 * mn64


# ---- argument validation -------------------------------------------------------------------
def _tri_call():
    s = lc.scene("sideways", 0.5, 63)
    n = len(s["pairs"])
    a = dict(k1=s["KF1"].cstruct(), k2=s["KF2"].cstruct(), d1=s["depth1"].copy(), d2=s["depth2"].copy(),
             s2=s["sigma2"].copy(), pairs=s["pairs"].copy(), x3D=np.zeros((n, 3), np.float32),
             status=np.zeros(n, np.int8), keys1=s["KF1"].keysUn.copy(), keys2=s["KF2"].keysUn.copy())
    a["k1"].keysUn, a["k2"].keysUn = a["keys1"].ctypes.data, a["keys2"].ctypes.data
    q = orb_triangulate()
    q.KF2 = C.pointer(a["k2"])
    q.depth2, q.levelSigma2_2, q.npairs = ptr(a["d2"]), ptr(a["s2"]), n
    q.pairs, q.x3D, q.status = ptr(a["pairs"]), ptr(a["x3D"]), ptr(a["status"])
    a["q"] = q
    return a


def _handle():
    """A matcher where a device exists; NULL otherwise (validation comes before the handle)."""
    return orb.ORBmatcher(0.6, True) if orb.device_available() else None


def test_create_new_map_points_validates_before_the_device():
    call = lib().LocalMapping_CreateNewMapPoints_batch
    m = _handle()
    h = m._h if m else None

    def run(a, count=1, kf1=True, d1=True, s2=True, nb=True):
        return call(h, C.byref(a["k1"]) if kf1 else None, ptr(a["d1"]) if d1 else None,
                    ptr(a["s2"]) if s2 else None, 1.2, count, C.byref(a["q"]) if nb else None)

    a = _tri_call()
    assert run(a, kf1=False) == ORB_E_INVALID
    assert run(a, d1=False) == ORB_E_INVALID          # KF1 has uRight: mvDepth is required
    assert run(a, s2=False) == ORB_E_INVALID
    assert run(a, nb=False) == ORB_E_INVALID
    assert run(a, count=-1) == ORB_E_INVALID
    for field in ("KF2", "depth2", "levelSigma2_2", "pairs", "x3D", "status"):
        a = _tri_call()
        setattr(a["q"], field, None)
        assert run(a) == ORB_E_INVALID, field
    a = _tri_call()
    a["q"].npairs = -1
    assert run(a) == ORB_E_INVALID
    a = _tri_call()
    a["q"].normal = ptr(np.zeros((63, 3), np.float32))       # the optional outputs come together
    assert run(a) == ORB_E_INVALID
    for col, val in ((0, -1), (0, 63), (1, -1), (1, 63)):      # pair indices outside [0, N)
        a = _tri_call()
        a["pairs"][5, col] = val
        assert run(a) == ORB_E_INVALID, (col, val)
    for keys, col, val in (("keys1", 0, -1), ("keys1", 0, 8), ("keys2", 1, -1), ("keys2", 1, 8)):
        a = _tri_call()                                        # octaves outside [0, nlevels)
        a[keys]["octave"][a["pairs"][7, col]] = val
        assert run(a) == ORB_E_INVALID, (keys, val)
    a = _tri_call()
    if not orb.device_available():
        assert run(a) == ORB_E_NODEVICE
        assert run(a, count=0, nb=False) == ORB_E_NODEVICE
    else:
        assert run(a) == 0
        assert call(None, C.byref(a["k1"]), ptr(a["d1"]), ptr(a["s2"]), 1.2, 1, C.byref(a["q"])) == ORB_E_INVALID


def _upd_call(ks=(0, 1, 2, 5)):
    c = lc.update_case(list(ks))
    n = len(ks)
    a = {k: v.copy() for k, v in c.items()}
    a.update(best=np.zeros(n, np.int32), normal=np.zeros((n, 3), np.float32), max_dist=np.zeros(n, np.float32),
             min_dist=np.zeros(n, np.float32))
    U = orb_pointupdate()
    U.npts = n
    for f in ("obs_start", "obs_desc", "best", "pos", "obs_Ow", "ref_Ow", "ref_scale", "ref_scale_top", "normal",
              "max_dist", "min_dist"):
        setattr(U, f, ptr(a[f]))
    return a, U


def test_map_point_update_validates_before_the_device():
    call = lib().MapPoint_Update_batch
    m = _handle()
    h = m._h if m else None
    assert call(h, None) == ORB_E_INVALID
    a, U = _upd_call()
    U.npts = -1
    assert call(h, C.byref(U)) == ORB_E_INVALID
    for field in ("obs_start", "best", "obs_Ow", "ref_Ow", "ref_scale", "ref_scale_top", "normal", "max_dist",
                  "min_dist"):
        a, U = _upd_call()
        setattr(U, field, None)
        assert call(h, C.byref(U)) == ORB_E_INVALID, field
    a, U = _upd_call()
    a["obs_start"][2] = 0                                      # non-monotone: 0 0 0 3 8 -> 0 0 1 0 ...
    a["obs_start"][1] = 1
    assert call(h, C.byref(U)) == ORB_E_INVALID
    a, U = _upd_call()
    a["obs_start"][0] = 1
    assert call(h, C.byref(U)) == ORB_E_INVALID
    a, U = _upd_call()
    if not orb.device_available():
        assert call(h, C.byref(U)) == ORB_E_NODEVICE
        with pytest.raises(orb.OrbGpuError) as ei:
            orb.ORBmatcher(0.6, True)
        assert ei.value.code == ORB_E_NODEVICE
    else:
        assert call(h, C.byref(U)) == 0
        assert call(None, C.byref(U)) == ORB_E_INVALID
