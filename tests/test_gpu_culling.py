"""LocalMapping_KeyFrameCulling / LocalMapping_MapPointCulling on the device against the restatement
(tests/culling_ref.py).  Everything is integer work and one float comparison whose operands are exact: every
output is compared for equality.  Shapes are the smallest that reach each path: rows of 0, 1, 10-200 and 4096
slots (one and sixteen passes of a 256-lane workgroup), 3-150 keyframes, a point list longer than a wave."""
import ctypes as C

import numpy as np
import pytest

import culling_cases as cc
import map_cases as mc
from c_orb_slam_amd._lib import ORB_E_CAPACITY, ORB_E_INVALID, lib, orb_kfcull, ptr
from culling_ref import CullRefMap

pytestmark = pytest.mark.gpu


@pytest.fixture()
def knobs():
    L = lib()
    yield L
    L.orbgpu_unit_set_map_initial_capacity(0, 0, 0)


class Pair:
    """A library Map and a CullRefMap that receive the same calls."""

    def __init__(self, gpu, ops=(), n_pts=0):
        self.map, self.ref, self.n_pts = gpu.Map(), CullRefMap(), n_pts
        self.apply(ops)

    def apply(self, ops):
        mc.apply(self.map, ops)
        mc.apply(self.ref, ops)

    def live(self):
        return sorted(k for k, kf in self.ref.kfs.items() if not kf.isBad())

    def cull(self, cand, not_erase=None, monocular=True, apply=True, **kw):
        """KeyFrameCulling on both; -> the library's result, equal to the restatement's.  With apply=False the
        restatement has moved on and the library has not."""
        bad = self.ref.bad_flags(self.n_pts) if self.n_pts else None
        got = self.map.KeyFrameCulling(cand, not_erase, monocular, bad=bad, apply=apply, **kw)
        want = self.ref.KeyFrameCulling(cand, not_erase, monocular)
        for k in ("nMPs", "nRedundant", "verdict", "bad_mp"):
            assert got[k].tolist() == want[k], k
        return got

    def catch_up(self, cand, got):
        """What an adapter does after apply=0."""
        for c, v in zip(cand, got["verdict"]):
            if v == 1:
                self.map.EraseKeyFrame(int(c))
        for p in got["bad_mp"]:
            self.map.EraseMapPoint(int(p))

    def check_state(self):
        n_kf, _, n_obs = self.map.size()
        assert n_kf == len(self.live())
        assert n_obs == sum(len(m.mObservations) for m in self.ref.pts.values())
        ids = self.live()
        for k, g in zip(ids, self.map.UpdateConnections_batch(ids)):
            assert tuple(x.tolist() for x in g) == tuple(self.ref.UpdateConnections(k)), k

    def cull_points(self, args, cur_kf, monocular, apply=True):
        bad = self.ref.bad_flags(self.n_pts)
        v, ob = self.map.MapPointCulling(*args, cur_kf, monocular, bad=bad, apply=apply)
        wv, wob = self.ref.MapPointCulling(*args, cur_kf, monocular)
        assert v.tolist() == wv and ob.tolist() == wob
        return v, ob


def shared_ops(n_pts, n_red, helpers=3, first_id=1):
    ops = [("AddKeyFrame", first_id, np.arange(n_pts, dtype=np.int32), None)]
    ops += [("AddKeyFrame", first_id + 1 + k, np.arange(n_red, dtype=np.int32), None) for k in range(helpers)]
    return ops


def test_known_answers_on_the_device(gpu):
    """The hand-computed answers of test_culling_cpu.py, asked of the library."""
    for n_pts, n_red, verdict in ((10, 9, 0), (10, 10, 1), (20, 18, 0), (20, 19, 1)):
        g = Pair(gpu, shared_ops(n_pts, n_red)).cull([1])
        assert (g["nMPs"].tolist(), g["nRedundant"].tolist(), g["verdict"].tolist()) == ([n_pts], [n_red], [verdict])
    for top, want in ((3, 1), (4, 0)):                                  # octave level + 1 and level + 2
        p = Pair(gpu, shared_ops(1, 1) + [("SetKeyFrameKeys", k, [o]) for k, o in ((1, 2), (2, 3), (3, 0), (4, top))])
        assert p.cull([1])["verdict"].tolist() == [want]
    p = Pair(gpu, shared_ops(1, 1, helpers=1) + [("SetKeyFrameKeys", k, [0], [5.0]) for k in (1, 2)])
    assert p.cull([1])["nRedundant"].tolist() == [0]                    # two stereo observers
    p = Pair(gpu, [("AddKeyFrame", 1, np.array([0], np.int32), np.array([0], np.uint8))] +
             [("AddKeyFrame", k, np.array([0], np.int32), None) for k in (2, 3, 4)])
    g = p.cull([1])                                                     # the candidate's own slot unobserved
    assert (g["nMPs"].tolist(), g["nRedundant"].tolist(), g["verdict"].tolist()) == ([1], [0], [0])
    far = [("SetKeyFrameKeys", 1, [0] * 4, [1.0, 1.0, 1.0, -1.0], [5.0, 40.0, 40.5, -1.0], 40.0)]
    g = Pair(gpu, shared_ops(4, 2) + far).cull([1], monocular=False)
    assert (g["nMPs"].tolist(), g["nRedundant"].tolist(), g["verdict"].tolist()) == ([2], [2], [1])
    g = Pair(gpu, shared_ops(4, 2) + far).cull([1], monocular=True)
    assert (g["nMPs"].tolist(), g["nRedundant"].tolist(), g["verdict"].tolist()) == ([4], [2], [0])
    # an empty row, a row of no slots, id 0, an erased id, an unknown id, not_erase
    p = Pair(gpu, shared_ops(10, 10) + [("AddKeyFrame", 0, np.arange(10, dtype=np.int32), None),
                                        ("AddKeyFrame", 7, np.full(5, -1, np.int32), None),
                                        ("AddKeyFrame", 8, np.zeros(0, np.int32), None),
                                        ("AddKeyFrame", 9, np.arange(10, dtype=np.int32), None), ("EraseKeyFrame", 9)])
    g = p.cull([7, 8, 0, 9, 55, 1], np.array([0, 0, 0, 0, 0, 1], np.uint8))
    assert g["verdict"].tolist() == [0, 0, 3, 3, 3, 2] and g["nMPs"].tolist() == [0, 0, 0, 0, 0, 10]
    assert p.map.size()[0] == 7
    assert p.cull([1], np.array([0], np.uint8))["verdict"].tolist() == [1] and p.map.size()[0] == 6
    # a cull breaks redundancy; a cull creates it; the order matters
    ops, cand = cc.gadget_break(1, 0)
    g = Pair(gpu, ops).cull(cand)
    assert g["verdict"].tolist() == [1, 0] and g["nRedundant"].tolist() == [10, 0] and len(g["bad_mp"]) == 0
    ops, cand = cc.gadget_create(1, 100)
    g = Pair(gpu, ops).cull(cand)
    assert g["verdict"].tolist() == [1, 1] and g["nMPs"].tolist() == [21, 10] and g["bad_mp"].tolist() == [119, 120]
    assert Pair(gpu, ops).cull(cand[1:])["verdict"].tolist() == [0]
    g = Pair(gpu, ops).cull(cand[::-1])
    assert g["verdict"].tolist() == [0, 1] and g["bad_mp"].tolist() == [119, 120]


@pytest.mark.parametrize("name", list(cc.FAMILIES))
def test_generated_family_matches_restatement(gpu, name):
    ops, calls, n_pts = cc.family(name)
    p = Pair(gpu, ops, n_pts)
    for cand, ne, mono in calls:
        p.cull(cand, ne, mono, apply=True)
        p.check_state()
    # the same sensor's other mode over what is left, without applying; then the adapter's way
    cand = np.array(p.live()[:140], np.int32)
    g = p.cull(cand, None, not calls[0][2], apply=False)
    p.catch_up(cand, g)
    p.check_state()


def test_keys_never_set_read_as_octave_0_monocular_not_far(gpu):
    ops = [op for op in cc.gen_cull_map(9, 20, 96, 90, 10, stereo=True) if op[0] == "AddKeyFrame"]
    p = Pair(gpu, ops, 400)
    g = p.cull(np.arange(1, 20, dtype=np.int32), None, False)
    assert 1 in g["verdict"].tolist() and g["nMPs"].max() > 60             # no slot is far
    p.check_state()
    L, oc = lib(), np.zeros(96, np.uint8)
    assert L.Map_SetKeyFrameKeys(p.map._h, 77, 96, ptr(oc), None, None, 0.0) == ORB_E_INVALID     # an unknown id
    assert L.Map_SetKeyFrameKeys(p.map._h, 0, 95, ptr(oc), None, None, 0.0) == ORB_E_INVALID     # another N
    assert L.Map_SetKeyFrameKeys(p.map._h, 0, 96, ptr(oc), None, None, 0.0) == 0


def test_point_with_more_than_64_observers_and_flagged_points(gpu):
    """Point 0 sits in 100 rows with octaves on both sides of every level; a tenth of the points are flagged bad
    in the caller's table while the handle still holds them."""
    rng = np.random.default_rng(3)
    ops = cc.gen_cull_map(11, 100, 64, 60, 3, fill=0.9, spread=0.4)
    for op in ops:
        if op[0] == "AddKeyFrame":
            row = op[2]
            row[row == 0] = -1
            row[int(rng.integers(0, 64))] = 0
    p = Pair(gpu, ops, 400)
    assert len(p.ref.pts[0].mObservations) > 64
    for q in rng.permutation(np.arange(1, 360))[:36]:
        p.ref.point(int(q)).mbBad = True
    g = p.cull(np.arange(1, 100, dtype=np.int32), None, True, apply=False)
    assert 1 in g["verdict"].tolist() and 0 in g["verdict"].tolist()


def test_rows_of_4096_1_and_0_slots(gpu):
    rng = np.random.default_rng(5)
    ops = []
    for k in range(1, 6):                                                  # five rows of 4096 over 4300 points
        mp = rng.permutation(4300)[:4096].astype(np.int32)
        ops += [("AddKeyFrame", k, mp, (rng.random(4096) < 0.97).astype(np.uint8)),
                ("SetKeyFrameKeys", k, np.ones(4096, np.uint8)) + cc.keys(rng, 4096, True)[1:]]
    ops += [("AddKeyFrame", 6, np.array([17], np.int32), None), ("AddKeyFrame", 7, np.zeros(0, np.int32), None)]
    for mono in (True, False):
        p = Pair(gpu, ops, 4300)
        g = p.cull(np.array([6, 1, 7, 2, 3, 4, 5], np.int32), None, mono)
        # a point of a big row has three of the four others with probability 0.96, all three of three with 0.78
        assert g["verdict"].tolist() == [1, 1, 0, 0, 0, 0, 0] and g["nMPs"][1] > (3000 if mono else 1000)
        p.check_state()


def test_more_than_128_candidates_and_a_chain_of_culls(gpu):
    """150 candidates in one call; 30 keyframes over the same 50 points are culled one after another until four
    are left, and the fourth last goes as well (three others remain)."""
    ops, _, n_pts = cc.family("many_keyframes")
    p = Pair(gpu, ops, n_pts)
    cand = np.arange(150, dtype=np.int32)[::-1].copy()
    g = p.cull(cand, None, False)
    assert len(cand) > 128 and g["verdict"].tolist().count(1) > 20 and g["verdict"][-1] == 3
    p.check_state()
    pts = np.arange(50, dtype=np.int32)
    q = Pair(gpu, [("AddKeyFrame", k, pts, None) for k in range(1, 31)])
    g = q.cull(np.arange(1, 31, dtype=np.int32))
    assert g["verdict"].tolist() == [1] * 27 + [0] * 3 and len(g["bad_mp"]) == 0
    assert g["nRedundant"].tolist() == [50] * 27 + [0] * 3
    q.check_state()


def test_apply_0_leaves_the_handle_unchanged(gpu):
    ops, calls, n_pts = cc.family("dense_mono")
    p = Pair(gpu, ops, n_pts)
    cand, ne, mono = calls[0]
    size = p.map.size()
    first = p.map.KeyFrameCulling(cand, ne, mono, apply=False)
    assert p.map.size() == size and first["verdict"].tolist().count(1) > 2 and len(first["bad_mp"]) > 1
    again = p.cull(cand, ne, mono, apply=False)
    assert all(np.array_equal(first[k], again[k]) for k in first) and p.map.size() == size
    p.catch_up(cand, again)
    p.check_state()


def test_capacity_is_reported_and_nothing_written_or_applied(gpu):
    ops, cand = cc.gadget_create(1, 100)
    p = Pair(gpu, ops)
    size = p.map.size()
    L = lib()
    cand = np.array(cand, np.int32)
    out = [np.full(4, -77, np.int32) for _ in range(4)]
    r = orb_kfcull(2, ptr(cand), None, 1, None, 0, 1, 1, *(ptr(o) for o in out), 0)
    assert L.LocalMapping_KeyFrameCulling(p.map._h, C.byref(r)) == ORB_E_CAPACITY
    assert r.n_bad == 2 and out[3].tolist() == [119, -77, -77, -77] and out[2].tolist()[:2] == [1, 1]
    assert p.map.size() == size                                            # nothing applied
    g = p.map.KeyFrameCulling(cand, None, True, cap_bad=1, apply=False)   # the wrapper asks again
    assert g["bad_mp"].tolist() == [119, 120]
    p.cull(cand, None, True, cap_bad=2)
    p.check_state()


def test_culling_after_each_kind_of_mutation_from_tiny_capacities(gpu, knobs):
    """The handle starts with room for 4 keyframes, 256 slots and 64 point ids; every pool grows, rows move in
    repacks and into reused storage, and the keys follow them."""
    knobs.orbgpu_unit_set_map_initial_capacity(4, 256, 64)
    ops = cc.gen_cull_map(21, 40, 96, 90, 8, fill=0.95, stereo=True)
    n_pts = 500
    p = Pair(gpu, ops, n_pts)
    rows = {k: [m.mnId if m else -1 for m in kf.mvpMapPoints] for k, kf in p.ref.kfs.items()}
    p.cull(np.array([5, 6], np.int32), None, False, apply=False)          # builds the index once
    p.ref = CullRefMap()
    mc.apply(p.ref, ops)
    held = [i for i, v in enumerate(rows[12]) if v >= 0]
    free = [i for i, v in enumerate(rows[12]) if v < 0]
    p.apply([("SetMapPointMatches", 12, np.array(held[:20], np.int32), np.full(20, -1, np.int32), None),
             ("SetMapPointMatches", 12, np.array(free[:2], np.int32), np.array([480, 481], np.int32),
              np.array([0, 1], np.uint8)),
             ("SetMapPointMatches", 12, np.array([held[30], free[3]], np.int32),
              np.array([-1, rows[12][held[30]]], np.int32), None)])
    p.cull(np.array([12, 11, 13], np.int32), None, False)
    p.check_state()
    seen = lambda k: {q for q, m in p.ref.pts.items() if p.ref.kfs[k] in m.mObservations}
    both = sorted(seen(20) & seen(21))
    only20 = sorted(seen(20) - set(rows[21]))
    p.apply([("EraseMapPoint", both[0]), ("EraseMapPoint", both[1]), ("ReplaceMapPoint", both[2], only20[0])])
    p.cull(np.array([21, 20, 19, 22], np.int32), None, False)
    p.check_state()
    # most keyframes erased: the rows that are left move in a repack; new keyframes take the freed storage
    p.apply([("EraseKeyFrame", k) for k in p.live() if k % 5 != 0 and k > 3])
    octs = {k: list(p.ref.kfs[k].octave) for k in p.live()}
    p.cull(np.array(p.live(), np.int32), None, True)
    extra = cc.gen_cull_map(22, 12, 96, 90, 8, fill=0.95, stereo=True, first_id=41)
    p.apply(extra)
    p.apply([("SetKeyFrameKeys", 41, np.full(96, 7, np.uint8), None, None, 0.0)])   # keys set again
    g = p.cull(np.arange(53, 0, -1, dtype=np.int32), None, False)
    assert 1 in g["verdict"].tolist()
    assert all(list(p.ref.kfs[k].octave) == v for k, v in octs.items())
    p.check_state()
    p.map.clear()
    p.ref = CullRefMap()
    p.apply(cc.gen_cull_map(23, 6, 64, 60, 4, fill=1.0))                  # after clear: fresh keys
    assert 3 not in p.cull(np.arange(1, 6, dtype=np.int32))["verdict"].tolist()
    p.check_state()


def test_update_local_map_and_culling_interleaved(gpu):
    ops, calls, n_pts = cc.family("dense_stereo")
    p = Pair(gpu, ops, n_pts)
    m = gpu.ORBmatcher(0.8, False)
    frames = mc.gen_frames(3, p.ref, 3, 300, n_pts)
    ask = lambda: m.UpdateLocalMap(p.map, [f.copy() for f in frames], kf_cap=64, pt_cap=n_pts)
    cand, ne, mono = calls[0]
    want = [p.ref.UpdateLocalMap([int(x) for x in f]) for f in frames]
    local0 = ask()
    cull0 = p.map.KeyFrameCulling(cand, ne, mono, apply=False)
    local1 = ask()
    cull1 = p.cull(cand, ne, mono, apply=False)
    for a, b in zip(local0, local1):
        assert all(np.array_equal(a[k], b[k]) for k in ("local_kf", "local_mp", "cur_row")) and a["n_kf"] > 0
    assert all(np.array_equal(cull0[k], cull1[k]) for k in cull0)
    for a, w in zip(local0, want):
        assert a["local_kf"].tolist() == w["local_kf"] and a["local_mp"].tolist() == w["local_mp"]


@pytest.mark.parametrize("monocular", [True, False])
def test_map_point_culling_matches_restatement(gpu, monocular):
    ops, calls, n_pts = cc.family("dense_mono" if monocular else "dense_stereo")
    p = Pair(gpu, ops, n_pts + 50)
    p.apply([("EraseMapPoint", q) for q in range(40, 60)])               # isBad() rows of the caller's table
    args = cc.gen_point_lists(7, n_pts + 50, 600, 12)                      # the last 50 ids were never observed
    v0, ob0 = p.map.MapPointCulling(*args, 12, monocular, bad=p.ref.bad_flags(p.n_pts), apply=False)
    size = p.map.size()
    v, ob = p.cull_points(args, 12, monocular, apply=True)
    assert np.array_equal(v, v0) and np.array_equal(ob, ob0) and p.map.size() != size
    assert set(v.tolist()) == {0, 1, 2, 3, 4} and ob.max() > 6 and (ob[args[0] >= n_pts] == 0).all()
    p.check_state()
    # the known answers of test_culling_cpu.py
    small = [("AddKeyFrame", 1 + k, np.arange(6 - k, dtype=np.int32), None) for k in range(4)] + [("EraseMapPoint", 0)]
    v, ob = Pair(gpu, small, 100).cull_points(([0, 1, 3, 2, 2, 5, 77], [10, 10, 8, 7, 9, 5, 8], [0, 1, 9, 9, 9, 0, 9],
                           [9, 5, 9, 9, 9, 9, 9]), 10, False, apply=False)
    assert v.tolist() == [1, 2, 3, 4, 0, 2, 3] and ob.tolist() == [0, 4, 3, 4, 4, 1, 0]
    v, _ = Pair(gpu, small, 100).cull_points(([1, 1], [10, 10], [1, 2], [4, 9]), 10, False, apply=False)
    assert v.tolist() == [0, 2]
