"""Map without a device: hand-computed known answers for the restatement (tests/map_ref.py) -- each
small enough to follow on paper, and none of them computed by the code under test -- and the
argument validation of the Map entries, which answers before a device is touched."""
import ctypes as C

import numpy as np

from c_orb_slam_amd._lib import (ORB_E_INVALID, ORB_E_NODEVICE, device_available, lib, orb_connections,
                                 orb_localupdate, ptr)
from map_ref import RefMap


def i32(*a):
    return np.array(a, np.int32)


def test_vote_tie_takes_the_lowest_id():
    r = RefMap()
    r.AddKeyFrame(5, i32(1, 0, 2))
    r.AddKeyFrame(3, i32(0, 1))
    cur = [0, 1]
    g = r.UpdateLocalMap(cur)
    # both keyframes get two votes; ids ascend; the first strict maximum is 3
    assert g["local_kf"] == [3, 5] and g["ref_kf"] == 3
    # rows in list order: kf 3 gives 0, 1; kf 5 adds 2
    assert g["local_mp"] == [0, 1, 2] and g["cur_row"] == [0, 1] and cur == [0, 1]


def test_weight_tie_in_the_ordered_list_puts_the_larger_id_first():
    r = RefMap()
    pts = np.arange(16, dtype=np.int32)
    r.AddKeyFrame(1, pts)
    r.AddKeyFrame(2, pts)
    r.AddKeyFrame(4, pts)
    cid, cn, oid, ow = r.UpdateConnections(1)
    assert (cid, cn) == ([2, 4], [16, 16])
    assert (oid, ow) == ([4, 2], [16, 16])


def test_no_weight_reaches_15_keeps_the_single_first_maximum():
    r = RefMap()
    r.AddKeyFrame(1, i32(0, 1, 2, 3))
    r.AddKeyFrame(2, i32(0, 1))
    r.AddKeyFrame(3, i32(2, 3))
    cid, cn, oid, ow = r.UpdateConnections(1)
    assert (cid, cn) == ([2, 3], [2, 2])
    assert (oid, ow) == ([2], [2])
    # and a keyframe that shares nothing has no connection at all
    r.AddKeyFrame(9, i32(50))
    assert r.UpdateConnections(9) == ([], [], [], [])


def test_parent_break_ends_the_whole_extension():
    r = RefMap()
    r.AddKeyFrame(1, i32(0))
    r.AddKeyFrame(2, i32(1))
    r.AddKeyFrame(10, i32(7))
    r.AddKeyFrame(11, i32(8))
    r.SetNeighbours(1, [], parent=10)
    r.SetNeighbours(2, [11])
    g = r.UpdateLocalMap([0, 1])
    # kf 1 appends its parent 10 and the loop ends: kf 2's covisible 11 is never looked at
    assert g["local_kf"] == [1, 2, 10] and g["ref_kf"] == 1
    assert g["local_mp"] == [0, 1, 7]
    # without the parent, kf 2 gets its turn
    r.SetNeighbours(1, [], parent=-1)
    assert r.UpdateLocalMap([0, 1])["local_kf"] == [1, 2, 11]


def test_extension_stops_above_80_keyframes():
    r = RefMap()
    for k in range(81):
        r.AddKeyFrame(k, i32(0))
        r.AddKeyFrame(100 + k, i32(1 + k))
    for k in range(81):
        r.SetNeighbours(k, [100 + k])
    # 81 voted keyframes: the list already holds more than 80, nothing is appended
    assert r.UpdateLocalMap([0])["local_kf"] == list(range(81))
    # 80 voted: the first iteration still runs (80 is not more than 80), the second does not
    r.EraseKeyFrame(80)
    assert r.UpdateLocalMap([0])["local_kf"] == list(range(80)) + [100]


def test_neighbour_already_voted_is_passed_over():
    r = RefMap()
    r.AddKeyFrame(1, i32(0))
    r.AddKeyFrame(2, i32(1))
    r.AddKeyFrame(3, i32(2))
    r.SetNeighbours(1, [2, 3])
    r.SetNeighbours(2, [1])
    g = r.UpdateLocalMap([0, 1])
    assert g["local_kf"] == [1, 2, 3] and g["local_mp"] == [0, 1, 2]


def test_point_held_by_two_keypoints_votes_twice():
    r = RefMap()
    r.AddKeyFrame(1, i32(1))
    r.AddKeyFrame(2, i32(0))
    # once each would be a tie for kf 1; point 0 twice makes kf 2 the strict maximum
    assert r.UpdateLocalMap([0, 1])["ref_kf"] == 1
    g = r.UpdateLocalMap([0, 0, 1])
    assert g["ref_kf"] == 2 and g["local_kf"] == [1, 2]
    assert g["local_mp"] == [1, 0] and g["cur_row"] == [1, 1, 0]


def test_unobserved_slot_does_not_vote_but_gives_a_local_point():
    r = RefMap()
    r.AddKeyFrame(1, i32(0, 1), np.array([1, 0], np.uint8))
    r.AddKeyFrame(2, i32(1))
    # point 1 is observed by kf 2 only: kf 1 holds it without the observation
    assert r.UpdateLocalMap([1])["local_kf"] == [2]
    # a vote for kf 1 through point 0 brings point 1 in as a local point all the same
    g = r.UpdateLocalMap([0])
    assert g["local_kf"] == [1] and g["local_mp"] == [0, 1]
    assert r.UpdateConnections(1)[0] == [2] and r.UpdateConnections(2)[0] == []


def test_empty_vote_returns_early_and_bad_points_are_cleared():
    r = RefMap()
    r.AddKeyFrame(1, i32(0, 3))
    assert r.UpdateLocalMap([-1, 5]) is None
    r.EraseMapPoint(3)
    cur = [3, -1]
    assert r.UpdateLocalMap(cur) is None and cur == [-1, -1]
    cur = [3, 0]
    g = r.UpdateLocalMap(cur)
    assert cur == [-1, 0] and g["local_mp"] == [0] and g["cur_row"] == [-1, 0]


def test_replace_takes_both_branches():
    r = RefMap()
    r.AddKeyFrame(1, i32(0, 1))
    r.AddKeyFrame(2, i32(0, 5))
    r.ReplaceMapPoint(0, 1)
    # kf 1 already holds point 1: its slot of point 0 is emptied; kf 2 takes point 1
    assert [m.mnId if m else -1 for m in r.kfs[1].mvpMapPoints] == [-1, 1]
    assert [m.mnId if m else -1 for m in r.kfs[2].mvpMapPoints] == [1, 5]
    assert r.UpdateConnections(1)[:2] == ([2], [1])


# ---------------------------------------------------------------- argument validation

def test_map_entries_validate_before_the_device():
    L = lib()
    mp = i32(1, 2, 3)
    assert L.Map_create(None) == ORB_E_INVALID
    assert L.Map_destroy(None) == ORB_E_INVALID
    assert L.Map_AddKeyFrame(None, 0, 4097, ptr(np.full(4097, -1, np.int32)), None) == ORB_E_INVALID
    assert L.Map_AddKeyFrame(None, 0, 3, ptr(i32(7, 2, 7)), None) == ORB_E_INVALID     # a point twice in the row
    assert L.Map_AddKeyFrame(None, -1, 3, ptr(mp), None) == ORB_E_INVALID
    assert L.Map_AddKeyFrame(None, 0, 3, None, None) == ORB_E_INVALID
    assert L.Map_SetMapPointMatches(None, 0, 2, ptr(i32(1, 1)), ptr(i32(4, 5)), None) == ORB_E_INVALID
    assert L.Map_SetMapPointMatches(None, 0, 2, ptr(i32(1, 2)), ptr(i32(4, 4)), None) == ORB_E_INVALID
    assert L.Map_EraseMapPoint(None, -1) == ORB_E_INVALID
    assert L.Map_ReplaceMapPoint(None, 1, -2) == ORB_E_INVALID
    assert L.Map_SetNeighbours(None, 0, 11, ptr(np.zeros(11, np.int32)), -1, 0, None) == ORB_E_INVALID
    r = orb_connections()
    r.cap_counter = 4                                                                   # without its arrays
    assert L.KeyFrame_UpdateConnections(None, 0, C.byref(r)) == ORB_E_INVALID
    assert L.KeyFrame_UpdateConnections(None, 0, None) == ORB_E_INVALID
    u = orb_localupdate()
    u.N = 4097
    assert L.Tracking_UpdateLocalMap_batch(None, None, 1, C.byref(u)) == ORB_E_INVALID
    assert L.Tracking_UpdateLocalMap_batch(None, None, 1, None) == ORB_E_INVALID
    assert L.Map_last_timings(None, None) == ORB_E_INVALID
    assert L.orbgpu_unit_set_map_initial_capacity(-1, 0, 0) == 1
    assert L.orbgpu_unit_set_map_chunk(-1) == 1
    assert L.orbgpu_unit_set_map_lds_slots(-2) == 1


def test_well_formed_calls_on_a_null_handle():
    L = lib()
    nodev = not device_available()
    NULL = ORB_E_NODEVICE if nodev else ORB_E_INVALID   # an otherwise valid call on a NULL handle
    if nodev:
        h = C.c_void_p()
        assert L.Map_create(C.byref(h)) == ORB_E_NODEVICE and not h.value
    mp = i32(1, 2, 3)
    assert L.Map_AddKeyFrame(None, 0, 3, ptr(mp), None) == NULL
    assert L.Map_SetMapPointMatches(None, 0, 1, ptr(i32(0)), ptr(i32(4)), None) == NULL
    assert L.Map_EraseMapPoint(None, 1) == NULL
    assert L.Map_ReplaceMapPoint(None, 1, 2) == NULL
    assert L.Map_EraseKeyFrame(None, 0) == NULL
    assert L.Map_clear(None) == NULL
    assert L.Map_size(None, None, None, None) == NULL
    assert L.Map_SetNeighbours(None, 0, 0, None, -1, 0, None) == NULL
    r = orb_connections()
    assert L.KeyFrame_UpdateConnections(None, 0, C.byref(r)) == NULL
    u = orb_localupdate()
    assert L.Tracking_UpdateLocalMap_batch(None, None, 1, C.byref(u)) == NULL
