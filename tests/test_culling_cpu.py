"""KeyFrameCulling / MapPointCulling without a device: known answers worked by hand against the restatement
(tests/culling_ref.py), the argument validation of the three new entries, which answers before a device is
touched, and the conditions that the generated families of the GPU tests must meet, evaluated on the restatement
alone."""
import copy
import ctypes as C

import numpy as np
import pytest

import culling_cases as cc
import map_cases as mc
from c_orb_slam_amd._lib import (ORB_E_INVALID, ORB_E_NODEVICE, device_available, lib, orb_kfcull, orb_pointcull,
                                 ptr)
from culling_ref import CullRefMap


def i32(*a):
    return np.array(a, np.int32)


def shared(n_pts, n_red, helpers=3):
    """Keyframe 1 holds points 0 .. n_pts-1; `helpers` more keyframes hold the first n_red of them.  All octave 0,
    monocular."""
    r = CullRefMap()
    r.AddKeyFrame(1, np.arange(n_pts, dtype=np.int32))
    for k in range(helpers):
        r.AddKeyFrame(2 + k, np.arange(n_red, dtype=np.int32))
    return r


# ---------------------------------------------------------------- KeyFrameCulling

@pytest.mark.parametrize("n_pts, n_red, verdict", [(10, 9, 0), (10, 10, 1), (20, 18, 0), (20, 19, 1)])
def test_the_tie_is_strict(n_pts, n_red, verdict):
    # 9 > 0.9 * 10 = 9.0 is false, 10 > 9.0 is true; 18 > 18.0 is false, 19 > 18.0 is true
    g = shared(n_pts, n_red).KeyFrameCulling([1], None, True)
    assert (g["nMPs"], g["nRedundant"], g["verdict"]) == ([n_pts], [n_red], [verdict])


def test_observer_octave_one_above_counts_and_two_above_does_not():
    for top, want in ((3, 1), (4, 0)):
        r = shared(1, 1)
        r.SetKeyFrameKeys(1, [2])
        r.SetKeyFrameKeys(2, [3])
        r.SetKeyFrameKeys(3, [0])
        r.SetKeyFrameKeys(4, [top])                       # level + 1 = 3 counts; 4 leaves two observers
        g = r.KeyFrameCulling([1], None, True)
        assert (g["nMPs"], g["nRedundant"], g["verdict"]) == ([1], [want], [want])


def test_two_stereo_observers_are_four_observations_but_one_other_observer():
    r = shared(1, 1, helpers=1)
    r.SetKeyFrameKeys(1, [0], [5.0])
    r.SetKeyFrameKeys(2, [0], [5.0])
    assert r.Observations(r.pts[0]) == 4
    g = r.KeyFrameCulling([1], None, True)
    assert (g["nMPs"], g["nRedundant"], g["verdict"]) == ([1], [0], [0])


def test_candidates_own_unobserved_slot_leaves_three_observations():
    r = CullRefMap()
    r.AddKeyFrame(1, i32(0), np.array([0], np.uint8))     # holds the point without the observation
    for k in (2, 3, 4):
        r.AddKeyFrame(k, i32(0))
    assert r.Observations(r.pts[0]) == 3                   # three qualifying others, but 3 > 3 is false
    g = r.KeyFrameCulling([1], None, True)
    assert (g["nMPs"], g["nRedundant"], g["verdict"]) == ([1], [0], [0])
    # with the observation there are four, and the three others make it redundant
    g = shared(1, 1).KeyFrameCulling([1], None, True)
    assert (g["nMPs"], g["nRedundant"], g["verdict"]) == ([1], [1], [1])


def test_far_slots_are_skipped_for_stereo_and_counted_when_monocular():
    def build():
        r = shared(4, 2)
        # slots 2 and 3 (not shared) are far: one beyond thDepth, one negative
        r.SetKeyFrameKeys(1, [0] * 4, [1.0, 1.0, 1.0, -1.0], [5.0, 40.0, 40.5, -1.0], 40.0)
        return r
    g = build().KeyFrameCulling([1], None, False)
    assert (g["nMPs"], g["nRedundant"], g["verdict"]) == ([2], [2], [1])
    g = build().KeyFrameCulling([1], None, True)
    assert (g["nMPs"], g["nRedundant"], g["verdict"]) == ([4], [2], [0])


def test_empty_row_id_zero_erased_id_and_not_erase():
    r = shared(10, 10)
    r.AddKeyFrame(0, np.arange(10, dtype=np.int32))       # id 0 would be redundant, and is never examined
    r.AddKeyFrame(7, np.full(5, -1, np.int32))
    r.AddKeyFrame(8, np.zeros(0, np.int32))
    r.AddKeyFrame(9, np.arange(10, dtype=np.int32))
    r.EraseKeyFrame(9)
    g = r.KeyFrameCulling([7, 8, 0, 9, 55, 1], [0, 0, 0, 0, 0, 1], True)
    assert g["verdict"] == [0, 0, 3, 3, 3, 2] and g["nMPs"] == [0, 0, 0, 0, 0, 10] and g["bad_mp"] == []
    assert r.live(1) is not None                           # mbToBeErased only
    g = r.KeyFrameCulling([1], [0], True)
    assert g["verdict"] == [1] and r.live(1) is None


def test_a_cull_breaks_redundancy():
    r = CullRefMap()
    ops, cand = cc.gadget_break(1, 0)
    mc.apply(r, ops)
    g = r.KeyFrameCulling(cand, None, True)
    # keyframe 1 goes; the points keep three observers, so keyframe 2 sees only two others per point
    assert cand == [1, 2] and g["verdict"] == [1, 0] and g["nMPs"] == [10, 10] and g["nRedundant"] == [10, 0]
    assert g["bad_mp"] == []


def test_a_cull_creates_redundancy_and_the_order_matters():
    def build():
        r = CullRefMap()
        ops, cand = cc.gadget_create(1, 100)
        mc.apply(r, ops)
        return r, cand
    r, cand = build()
    g = r.KeyFrameCulling(cand, None, True)
    assert g["verdict"] == [1, 1] and g["nMPs"] == [21, 10] and g["nRedundant"] == [19, 10]
    assert g["bad_mp"] == [119, 120]                       # A's slots 19 and 20, in slot order
    r, cand = build()
    g = r.KeyFrameCulling(cand[1:], None, True)            # B alone: 10 > 0.9 * 12 is false
    assert g["verdict"] == [0] and g["nMPs"] == [12] and g["nRedundant"] == [10]
    r, cand = build()
    g = r.KeyFrameCulling(cand[::-1], None, True)          # B first stays, A goes afterwards
    assert g["verdict"] == [0, 1] and g["bad_mp"] == [119, 120]


# ---------------------------------------------------------------- MapPointCulling

def test_map_point_culling_rules_and_their_precedence():
    r = CullRefMap()
    r.AddKeyFrame(1, i32(0, 1, 2, 3, 4, 5))
    r.AddKeyFrame(2, i32(0, 1, 2, 3, 4))
    r.AddKeyFrame(3, i32(0, 1, 2, 3))
    r.AddKeyFrame(4, i32(0, 1, 2))
    r.EraseMapPoint(0)
    #      bad  ratio  obs   old   keep  ratio-before-obs  never seen
    mp = [0, 1, 3, 2, 2, 5, 77]
    first = [10, 10, 8, 7, 9, 5, 8]
    found = [0, 1, 9, 9, 9, 0, 9]
    visible = [9, 5, 9, 9, 9, 9, 9]
    v, ob = copy.deepcopy(r).MapPointCulling(mp, first, found, visible, 10, False)
    # point 3 has 3 observations <= cnThObs 3 at age 2; point 2 has 4: age 3 drops it, age 1 keeps it
    assert v == [1, 2, 3, 4, 0, 2, 3] and ob == [0, 4, 3, 4, 4, 1, 0]
    # monocular: cnThObs is 2, so three observations survive rule 3
    v, _ = copy.deepcopy(r).MapPointCulling([3, 4], [8, 8], [9, 9], [9, 9], 10, True)
    assert v == [0, 3]
    # a quarter exactly is not below a quarter
    v, _ = copy.deepcopy(r).MapPointCulling([1, 1], [10, 10], [1, 2], [4, 9], 10, False)
    assert v == [0, 2]
    # SetBadFlag is run for verdicts 2 and 3 only
    q = copy.deepcopy(r)
    q.MapPointCulling(mp, first, found, visible, 10, False)
    assert [p for p in range(6) if q.pts[p].isBad()] == [0, 1, 3, 5]
    # a stereo observation counts 2: two stereo observers pass cnThObs 3
    r.SetKeyFrameKeys(1, [0] * 6, [1.0] * 6)
    r.SetKeyFrameKeys(2, [0] * 5, [1.0] * 5)
    v, ob = r.MapPointCulling([4], [8], [9], [9], 10, False)
    assert (v, ob) == ([0], [4])


# ---------------------------------------------------------------- argument validation

def _kfcull(n, ids, **kw):
    a = dict(nMPs=np.zeros(8, np.int32), nRedundant=np.zeros(8, np.int32), verdict=np.zeros(8, np.int32),
             bad_mp=np.zeros(8, np.int32))
    r = orb_kfcull()
    r.n, r.cand, r.cap_bad = n, ptr(ids), 8
    r.nMPs, r.nRedundant, r.verdict, r.bad_mp = (ptr(a[k]) for k in ("nMPs", "nRedundant", "verdict", "bad_mp"))
    for k, v in kw.items():
        setattr(r, k, v)
    return r, a


def test_culling_entries_validate_before_the_device():
    L = lib()
    oc = np.zeros(4, np.uint8)
    assert L.Map_SetKeyFrameKeys(None, -1, 4, ptr(oc), None, None, 0.0) == ORB_E_INVALID
    assert L.Map_SetKeyFrameKeys(None, 1, -1, ptr(oc), None, None, 0.0) == ORB_E_INVALID
    assert L.Map_SetKeyFrameKeys(None, 1, 4, None, None, None, 0.0) == ORB_E_INVALID
    assert L.Map_SetKeyFrameKeys(None, 1, 4097, ptr(np.zeros(4097, np.uint8)), None, None, 0.0) == ORB_E_INVALID
    assert L.LocalMapping_KeyFrameCulling(None, None) == ORB_E_INVALID
    cand = i32(3, 4, 3)
    for r, keep in (_kfcull(-1, cand), _kfcull(3, cand),                      # n < 0; a candidate twice
                    _kfcull(2, cand, cand=None), _kfcull(2, cand, verdict=None), _kfcull(2, cand, nMPs=None),
                    _kfcull(2, cand, nRedundant=None), _kfcull(2, cand, bad_mp=None), _kfcull(2, cand, cap_bad=-1),
                    _kfcull(2, cand, nbad=5)):                                  # bad flags without the array
        assert L.LocalMapping_KeyFrameCulling(None, C.byref(r)) == ORB_E_INVALID
    assert L.LocalMapping_MapPointCulling(None, None) == ORB_E_INVALID
    ok = dict(mp=i32(1, 2), first_kf=i32(0, 0), found=i32(1, 1), visible=i32(1, 1), verdict=i32(0, 0))
    for bad_key, bad_val in (("visible", i32(1, 0)), ("mp", i32(1, -1)), ("mp", None), ("verdict", None),
                             ("first_kf", None), ("found", None), ("visible", None)):
        a = dict(ok)
        a[bad_key] = bad_val
        r = orb_pointcull()
        r.n = 2
        r.mp, r.first_kf, r.found, r.visible, r.verdict = (ptr(a[k]) for k in ("mp", "first_kf", "found", "visible",
                                                                              "verdict"))
        assert L.LocalMapping_MapPointCulling(None, C.byref(r)) == ORB_E_INVALID, bad_key
    r = orb_pointcull()
    r.n = -1
    assert L.LocalMapping_MapPointCulling(None, C.byref(r)) == ORB_E_INVALID


def test_well_formed_culling_calls_on_a_null_handle():
    L = lib()
    NULL = ORB_E_NODEVICE if not device_available() else ORB_E_INVALID
    assert L.Map_SetKeyFrameKeys(None, 1, 4, ptr(np.zeros(4, np.uint8)), None, None, 0.0) == NULL
    r, keep = _kfcull(2, i32(3, 4))
    assert L.LocalMapping_KeyFrameCulling(None, C.byref(r)) == NULL
    a = dict(mp=i32(1, 2), first_kf=i32(0, 0), found=i32(1, 1), visible=i32(1, 1), verdict=i32(0, 0))
    p = orb_pointcull()
    p.n = 2
    p.mp, p.first_kf, p.found, p.visible, p.verdict = (ptr(a[k]) for k in ("mp", "first_kf", "found", "visible",
                                                                          "verdict"))
    assert L.LocalMapping_MapPointCulling(None, C.byref(p)) == NULL


# ---------------------------------------------------------------- the generated families

def state_before(ops, calls, k):
    """The restatement's map at the start of call k of a family."""
    ref = CullRefMap()
    mc.apply(ref, ops)
    for cand, ne, mono in calls[:k]:
        ref.KeyFrameCulling(cand, ne, mono)
    return ref


def test_generated_families_reach_every_kind_of_outcome():
    """What the GPU tests rely on the families for, checked on the restatement alone."""
    seen = set()
    for name in cc.FAMILIES:
        ops, calls, n_pts = cc.family(name)
        assert all(len(op[2]) <= 400 for op in ops if op[0] == "AddKeyFrame")
        assert 3 <= sum(op[0] == "AddKeyFrame" for op in ops) <= 160
        ref = state_before(ops, calls, 0)
        assert max(ref.pts) < n_pts
        for k, (cand, ne, mono) in enumerate(calls):
            g = ref.KeyFrameCulling(cand, ne, mono)
            seen |= {("verdict", v) for v in g["verdict"]}
            if 1 not in g["verdict"]:
                seen.add("no cull")
            if len(g["bad_mp"]) > 1:
                seen.add("several bad points")
            for i, c in enumerate(cand):
                if g["verdict"][i] in (0, 1) and 1 in g["verdict"][:i]:
                    alone = state_before(ops, calls, k).KeyFrameCulling([c], None if ne is None else [ne[i]], mono)
                    if alone["verdict"][0] != g["verdict"][i]:
                        seen.add(("initially", alone["verdict"][0], "then", g["verdict"][i]))
    for want in (("verdict", 0), ("verdict", 1), ("verdict", 2), ("verdict", 3), "no cull", "several bad points",
                 ("initially", 1, "then", 0), ("initially", 0, "then", 1)):
        assert want in seen, want
