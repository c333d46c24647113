"""The restatement of LoopClosing's map correction (tests/loopcorrect_ref.py) against properties that do not
depend on it, and against a float64 model.  No GPU is needed.

Tolerance.  The restatement rounds to float32 where the reference does; the float64 model does not.  Over
all cases of loopcorrect_cases.py the largest deviation between the two, in units of the float32 ulp of the
largest coordinate of the case (poses and positions together), was measured as 4.71 ulps (the pose at the
end of the 70-keyframe propagation chain, where the rounding of every step is carried along; the mixed
depth-5 tree reaches 3.61, every CorrectLoop case stays below 1.5).  The bound used below for the model and
for the invariants is four times that: 18.84 ulps.  It is there to catch a wrong restatement -- a wrong
association, a transposed rotation, a missed scale is off by thousands of ulps -- not to grade rounding."""
import math
import re

import numpy as np
import pytest

import loopcorrect_cases as lc
import loopcorrect_ref as lr
from c_orb_slam_amd import _lib

BOUND_ULPS = 4 * 4.71


@pytest.fixture(scope="module")
def correct():
    """name -> (case, RefMap, restatement result, quaternion branch counts of the run)"""
    out = {}
    for name, c in lc.correct_cases().items():
        lr.BRANCHES[:] = [0, 0, 0, 0]
        ref = c.refmap()
        out[name] = (c, ref, c.restate(ref), list(lr.BRANCHES))
    return out


@pytest.fixture(scope="module")
def gba():
    return {name: (c, c.refmap(), c.restate()) for name, c in lc.gba_cases().items()}


def ulp_of(*arrays):
    m = max(float(np.max(np.abs(a))) for a in arrays if np.size(a))
    return 2.0 ** (math.floor(math.log2(m)) - 23)


def dev(a, b, unit):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b))) / unit if a.size else 0.0


def T64(rows):
    return np.asarray(rows, np.float64).reshape(-1, 4, 4)


def cam(T, X):
    return T[:3, :3] @ X + T[:3, 3]


def model_deviations(correct, gba):
    """name -> ulps between the restatement and the float64 model"""
    out = {}
    for name, (c, ref, r, _) in correct.items():
        T, pos, who = lr.ref64_correct_loop(ref, c.kf, c.cur_kf, c.Scw, c.Tcw, c.pos, c.bad)
        assert {p: int(r["corrected_ref"][p]) for p in who} == who
        unit = ulp_of(r["Tcw"], r["pos"], c.pos)
        out["correct/" + name] = max(dev(r["Tcw"].reshape(-1, 4, 4), T, unit), dev(r["pos"], pos, unit))
    for name, (c, ref, r) in gba.items():
        T, pos = lr.ref64_apply_gba(ref, c.origins, c.TcwGBA, c.kf_in_gba, c.Tcw, c.pos, c.posGBA, c.mp_in_gba,
                                    c.ref_kf, c.bad)
        unit = ulp_of(r["Tcw"], r["pos"], c.pos) if c.n_pts else ulp_of(r["Tcw"])
        out["gba/" + name] = max(dev(r["Tcw"].reshape(-1, 4, 4), T, unit), dev(r["pos"], pos, unit))
    return out


def test_restatement_matches_the_float64_model(correct, gba):
    d = model_deviations(correct, gba)
    print({k: round(v, 2) for k, v in d.items()})
    assert max(d.values()) <= BOUND_ULPS, d


def test_corrected_points_keep_their_camera_coordinates_up_to_scale(correct):
    """In the corrector's new camera frame a corrected point sits at its old camera-frame place divided by s."""
    seen = 0
    for name, (c, ref, r, _) in correct.items():
        old, new = T64(c.Tcw), T64(r["Tcw"])
        order = {int(k): j for j, k in enumerate(c.kf)}
        unit = ulp_of(r["pos"], c.pos, r["Tcw"])
        for p in np.nonzero(r["corrected_ref"] != c.corrected_ref)[0]:
            k = int(r["corrected_ref"][p])
            s = float(r["CorrectedSim3"][order[k]][7])
            want = cam(old[k], c.pos[p].astype(np.float64)) / s
            got = cam(new[k], r["pos"][p].astype(np.float64))
            assert dev(got, want, unit) <= BOUND_ULPS, (name, p)
            seen += 1
    assert seen > 5000


def test_the_keyframes_own_sim3_brings_every_pose_back(correct):
    c, ref, r, _ = correct["identity"]
    listed = [int(k) for k in c.kf]
    unit = ulp_of(c.Tcw)
    assert dev(r["Tcw"][listed], c.Tcw[listed], unit) <= BOUND_ULPS
    others = [k for k in range(c.n_kf_rows) if k not in listed]
    assert np.array_equal(r["Tcw"][others], c.Tcw[others])
    assert np.allclose(r["CorrectedSim3"][:, 7], 1.0, rtol=0, atol=1e-12)


def test_propagated_keyframes_keep_their_pose_relative_to_the_parent(gba):
    seen = 0
    for name, (c, ref, r) in gba.items():
        old, new = T64(c.Tcw), T64(r["Tcw"])
        unit = ulp_of(r["Tcw"], c.Tcw)
        for k, kf in ref.kfs.items():
            par = kf.parent
            if not r["kf_done"][k] or c.kf_in_gba[k] or par < 0:
                continue
            want = old[k] @ np.linalg.inv(old[par])
            got = new[k] @ np.linalg.inv(new[par])
            assert dev(got, want, unit) <= BOUND_ULPS, (name, k)
            seen += 1
        assert seen == 0 or r["n_kf_propagated"] > 0
    assert seen >= 70 + 300


def test_moved_points_keep_their_place_in_the_reference_keyframe(gba):
    seen = 0
    for name, (c, ref, r) in gba.items():
        old, new = T64(c.Tcw), T64(r["Tcw"])
        if not c.n_pts:
            continue
        unit = ulp_of(r["pos"], c.pos, r["Tcw"])
        for p in range(c.n_pts):
            k = int(c.ref_kf[p])
            moved = not c.bad[p] and not c.mp_in_gba[p] and 0 <= k and r["kf_done"][k]
            if c.bad[p] or (not moved and not c.mp_in_gba[p]):
                assert np.array_equal(r["pos"][p], c.pos[p]), (name, p)
            elif c.mp_in_gba[p]:
                assert np.array_equal(r["pos"][p], c.posGBA[p]), (name, p)
            else:
                want = cam(old[k], c.pos[p].astype(np.float64))
                got = cam(new[k], r["pos"][p].astype(np.float64))
                assert dev(got, want, unit) <= BOUND_ULPS, (name, p)
                seen += 1
        assert seen == 0 or r["n_mp_moved"] > 0
    assert seen > 2500


def test_the_lowest_listed_id_corrects_a_point_held_by_all(correct):
    for name, (c, ref, r, _) in correct.items():
        holders = [int(k) for k in c.kf if 0 in ref.pts and ref.pts[0] in ref.kfs[int(k)].mvpMapPoints]
        if holders:
            assert r["corrected_ref"][0] == min(holders), name
    c, ref, r, _ = correct["seventy_listed"]
    assert len(ref.pts[0].mObservations) == 70 and r["corrected_ref"][0] == 3
    # points that nobody listed holds, and bad points, keep their mark and their row
    same = r["corrected_ref"] == c.corrected_ref
    assert same.any() and np.array_equal(r["pos"][same], c.pos[same]) and same[c.bad != 0].all()


def test_the_order_of_the_list_does_not_matter(correct):
    c, ref, r, _ = correct["three_listed_wide"]
    d = c.restate(ref, kf=np.sort(c.kf)[::-1].copy())
    for k in ("Tcw", "pos", "normal", "max_dist", "min_dist", "corrected_ref"):
        assert np.array_equal(r[k], d[k]), k
    back = {int(k): j for j, k in enumerate(np.sort(c.kf)[::-1])}
    assert np.array_equal(r["CorrectedSim3"], d["CorrectedSim3"][[back[int(k)] for k in c.kf]])


def test_every_quaternion_branch_is_taken(correct):
    total = np.sum([b for _, _, _, b in correct.values()], axis=0)
    assert (total > 0).all(), total.tolist()


def test_header_declares_and_binding_binds_the_entries():
    names = _lib.header_functions()
    src = (_lib.PKG / "_lib.py").read_text()
    for f in ("LoopClosing_CorrectLoop", "LoopClosing_ApplyGlobalBA"):
        assert f in names
        assert re.search(rf"L\.{f}\.argtypes", src)
    import c_orb_slam_amd
    assert hasattr(c_orb_slam_amd.LoopClosing, "CorrectLoop") and hasattr(c_orb_slam_amd.LoopClosing, "ApplyGlobalBA")
