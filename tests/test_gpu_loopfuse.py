"""LoopClosing_SearchAndFuse on the GPU against the literal restatement (tests/loopfuse_ref.py) over the cases
of tests/loopfuse_cases.py: nfused, the op log, updated, bad and the descriptor rows are equal byte for byte
(everything here is integers and bytes, so no tolerance is involved), and the handle moves as the
reference's map moves."""
import numpy as np
import pytest

import fuse_cases as fc
import loopfuse_cases as lc
from loopfuse_ref import SearchAndFuseRef, cvScw_of

pytestmark = pytest.mark.gpu

TABLE_OUT = ("desc", "bad")
TABLE_IN = ("pos", "normal", "max_dist", "min_dist")


@pytest.fixture(scope="module")
def reference():
    """name -> (RefMap after the run, the run): computed once, never changed by a test"""
    out = {}
    for name in lc.MAIN + lc.EDGE:
        c = lc.case(name)
        ref = c.refmap()
        out[name] = (ref, SearchAndFuseRef(ref, **c.kwargs(c.table)).run())
    return out


def run_library(gpu, c, table, m=None, mp=None, order=None, **kw):
    m = m or gpu.ORBmatcher(0.6, True)
    mp = mp or c.fill(gpu.Map())
    return m, mp, gpu.LoopClosing(m, mp).SearchAndFuse(**c.kwargs(table, order), **kw)


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_same_result(got, want, what):
    for k in ("nfused", "ops", "updated"):
        assert same_bytes(got[k], want[k]), (what, k, got[k][:12], want[k][:12])
    assert got["n_matched_skipped"] == want["n_matched_skipped"], what


def assert_same_table(t, want, what):
    for k in TABLE_OUT + TABLE_IN:
        if not same_bytes(t[k], want[k]):
            rows = np.flatnonzero((t[k].reshape(len(t[k]), -1) != want[k].reshape(len(t[k]), -1)).any(axis=1))
            raise AssertionError((what, k, rows[:8], t[k][rows[:3]], want[k][rows[:3]]))


def ref_size(ref):
    live = [kf for kf in ref.kfs.values() if not kf.isBad()]
    slots = sum(len(kf.mvpMapPoints) for kf in live)
    observed = sum(1 for kf in live for i, m in enumerate(kf.mvpMapPoints)
                   if m is not None and m.mObservations.get(kf) == i)
    return len(live), slots, observed


def assert_same_connections(mp, ref, ids, what):
    for kid, got in zip(ids, mp.UpdateConnections_batch(list(ids), cap_counter=64, cap_ordered=64)):
        want = ref.UpdateConnections(int(kid))
        assert all(np.array_equal(g, np.array(w, np.int32)) for g, w in zip(got, want)), (what, kid)


@pytest.mark.parametrize("name", lc.MAIN + lc.EDGE)
def test_parity_with_the_restatement(gpu, reference, name):
    c = lc.case(name)
    ref, r = reference[name]
    t = c.table_copy()
    m, mp, got = run_library(gpu, c, t)
    want = r.result()
    print(name, "nfused", got["nfused"].tolist(), "ops", len(got["ops"]), "updated", len(got["updated"]),
          "skipped", got["n_matched_skipped"])
    assert_same_result(got, want, name)
    assert_same_table(t, r.t, name)
    untouched = np.setdiff1d(np.arange(c.n_pts), got["updated"])
    for k in TABLE_OUT:
        assert same_bytes(t[k][untouched], c.table[k][untouched]), k
    assert mp.size() == ref_size(ref)


def test_one_keyframe_selects_what_fuse_sim3_selects(gpu):
    """Without step 0 the only pass meets the map as it was: its selection is ORBmatcher_Fuse_Sim3's."""
    from c_orb_slam_amd.orb import MapPointGeo, MapPoints
    c = lc.case("one_keyframe")
    t = c.table_copy()
    kw = c.kwargs(t)
    kw["matched"] = None
    m = gpu.ORBmatcher(0.6, True)
    mp = c.fill(gpu.Map())
    got = gpu.LoopClosing(m, mp).SearchAndFuse(**kw, apply=False)
    pKF = c.refmap().kfs[c.kf[0]]
    held = set(x.mnId for x in pKF.mvpMapPoints if x is not None and not c.table["bad"][x.mnId])
    loop = np.asarray(c.loop_pts)
    skip = np.array([p < 0 or bool(c.table["bad"][p]) or int(p) in held for p in loop], np.uint8)
    row = np.where(loop < 0, 0, loop)
    pts = MapPoints(c.table["pos"][row], c.table["desc"][row], np.ones(len(row), np.int32))
    geo = MapPointGeo(c.table["max_dist"][row], c.table["min_dist"][row], c.table["normal"][row])
    n, best = m.Fuse_Sim3(c.frames[0], cvScw_of(c.Scw[0]), pts, geo, skip, lc.LOG_SF, lc.TH)
    chosen = sorted(int(b) for b in best if b >= 0)
    assert n == got["nfused"][0] == len(got["ops"]) == len(chosen) and n > 50
    assert sorted(got["ops"][:, 5].tolist()) == chosen
    # adds and kind-3 ops are logged at the point's turn, in point order
    at_turn = got["ops"][got["ops"][:, 1] != 2]
    want, taken = [], set()
    for i, b in enumerate(int(x) for x in best):
        if b < 0:
            continue
        q = pKF.mvpMapPoints[b]
        if q is None and b not in taken:
            want.append((1, int(loop[i]), b))           # the first point at an empty keypoint is added
            taken.add(b)
        elif q is not None and c.table["bad"][q.mnId]:
            want.append((3, int(loop[i]), b))
    assert [(int(o[1]), int(o[2]), int(o[5])) for o in at_turn] == want and len(want) > 20


@pytest.mark.parametrize("name", ["stereo", "twice"])
def test_apply_1_moves_the_handle_as_the_reference_moves_the_map(gpu, reference, name):
    c = lc.case(name)
    ref0, r = reference[name]
    t = c.table_copy()
    m, mp, got = run_library(gpu, c, t, apply=True)
    assert mp.size() == ref_size(ref0)
    assert_same_connections(mp, ref0, sorted(c.kf), name)
    # a second call on what the first left (nothing is matched any more: step 0 is left out)
    ref2 = c.refmap()
    SearchAndFuseRef(ref2, **c.kwargs(c.table)).run()
    kw = c.kwargs(r.t)
    kw["matched"] = None
    r2 = SearchAndFuseRef(ref2, **kw).run()
    kw = c.kwargs(t)
    kw["matched"] = None
    got2 = gpu.LoopClosing(m, mp).SearchAndFuse(**kw, apply=True)
    assert_same_result(got2, r2.result(), name + " second run")
    assert_same_table(t, r2.t, name + " second run")
    assert mp.size() == ref_size(ref2)


def test_apply_0_leaves_the_handle_as_it_was(gpu, reference):
    c = lc.case("mono")
    t1, t2 = c.table_copy(), c.table_copy()
    m, mp, first = run_library(gpu, c, t1, apply=False)
    size = mp.size()
    assert size == ref_size(c.refmap())
    _, _, again = run_library(gpu, c, t2, m=m, mp=mp, apply=False)
    assert_same_result(again, first, "repeat")
    assert_same_table(t2, t1, "repeat")
    assert mp.size() == size
    assert_same_connections(mp, c.refmap(), sorted(c.kf), "apply 0")
    assert_same_result(first, reference["mono"][1].result(), "apply 0")


def test_capacity_one_short_writes_nothing(gpu, reference):
    from c_orb_slam_amd._lib import ORB_E_CAPACITY
    from c_orb_slam_amd.map import CapacityError
    c = lc.case("stereo")
    want = reference["stereo"][1].result()
    t = c.table_copy()
    m = gpu.ORBmatcher(0.6, True)
    mp = c.fill(gpu.Map())
    lcl = gpu.LoopClosing(m, mp)
    size = mp.size()
    for caps in ((len(want["ops"]) - 1, len(want["updated"])), (len(want["ops"]), len(want["updated"]) - 1)):
        with pytest.raises(CapacityError) as ei:
            lcl.SearchAndFuse(**c.kwargs(t), apply=True, cap_ops=caps[0], cap_updated=caps[1], retry=False)
        assert ei.value.code == ORB_E_CAPACITY
        assert (ei.value.n_ops, ei.value.n_updated) == (len(want["ops"]), len(want["updated"]))
        assert all(same_bytes(t[k], c.table[k]) for k in t)
        assert mp.size() == size
        assert_same_connections(mp, c.refmap(), sorted(c.kf), "after ORB_E_CAPACITY")
    got = lcl.SearchAndFuse(**c.kwargs(t), apply=True, cap_ops=len(want["ops"]), cap_updated=len(want["updated"]),
                            retry=False)
    assert_same_result(got, want, "with room")
    assert_same_table(t, reference["stereo"][1].t, "with room")
    got = gpu.LoopClosing(m, c.fill(gpu.Map())).SearchAndFuse(**c.kwargs(c.table_copy()), cap_ops=1, cap_updated=1)
    assert_same_result(got, want, "retried once")


def test_refusals(gpu):
    from c_orb_slam_amd._lib import ORB_E_INVALID, OrbGpuError, check, lib
    c = lc.case("one_keyframe")
    L = lib()

    def refused(m, mp, kw, table):
        before = {k: v.copy() for k, v in table.items()}
        size = mp.size()
        with pytest.raises(OrbGpuError) as ei:
            gpu.LoopClosing(m, mp).SearchAndFuse(**kw)
        assert ei.value.code == ORB_E_INVALID
        assert all(same_bytes(before[k], table[k]) for k in before) and mp.size() == size

    mp = c.fill(gpu.Map())
    t = c.table_copy()
    m = gpu.ORBmatcher(0.6, True)
    check(L.ORBmatcher_set_device_pointers(m._h, 1))
    refused(m, mp, c.kwargs(t), t)                                      # a device-pointer matcher
    check(L.ORBmatcher_set_deferred(m._h, 1))                           # (device-resident batches only)
    refused(m, mp, c.kwargs(t), t)                                      # a deferred matcher
    check(L.ORBmatcher_set_deferred(m._h, 0))
    m = gpu.ORBmatcher(0.6, True)
    kw = c.kwargs(t)
    kw.update(kf=kw["kf"] * 2, frames=kw["frames"] * 2, Scw=np.tile(kw["Scw"], (2, 1)))
    refused(m, mp, kw, t)                                               # a keyframe named twice
    kw = c.kwargs(t)
    loop = kw["loop_pts"].copy()
    held = np.flatnonzero(loop >= 0)
    loop[held[1]] = loop[held[0]]
    kw["loop_pts"] = loop
    refused(m, mp, kw, t)                                               # a duplicate loop id
    kw = c.kwargs(t)
    kw["kf"] = [13]
    refused(m, mp, kw, t)                                               # a listed id that is not live
    kw = c.kwargs(t)
    kw["matched"] = kw["matched"][:-1]
    refused(m, mp, kw, t)                                               # nmatched is not the row's size
    kw = c.kwargs(t)
    kw["kf_desc"] = {k: v for k, v in c.kf_desc.items() if k != c.base.ghost_ids[0]}
    refused(m, mp, kw, t)                                               # no descriptors for a live keyframe
    from c_orb_slam_amd.orb import Frame
    G = c.frames[0]
    kw = c.kwargs(t)
    kw["frames"] = [Frame(G.keysUn[:-1], G.desc[:-1], G.scale, G.Tcw, G.fx, G.fy, G.cx, G.cy, G.bf, fc.W, fc.H)]
    refused(m, mp, kw, t)                                               # N is not the row's size
    row = next(op[2] for op in c.base.ops if op[0] == "AddKeyFrame" and op[1] == c.kf[0])
    n = int(row.max())
    short = {k: v[:n].copy() for k, v in t.items()}
    kw = c.kwargs(short)
    kw["loop_pts"] = np.where(kw["loop_pts"] >= n, -1, kw["loop_pts"]).astype(np.int32)
    kw["matched"] = np.where(kw["matched"] >= n, -1, kw["matched"]).astype(np.int32)
    refused(m, mp, kw, short)                                           # a held id beyond the table
    mp2 = c.fill(gpu.Map())
    row = next(op[2] for op in c.base.ops if op[0] == "AddKeyFrame" and op[1] == c.kf[0])
    slot = int(np.flatnonzero(row >= 0)[0])
    mp2.SetMapPointMatches(c.kf[0], [slot], [int(row[slot])], observed=[0])
    refused(m, mp2, c.kwargs(t), t)                                     # a held but unobserved slot
    # and the untouched handle still serves the call
    got = gpu.LoopClosing(m, mp).SearchAndFuse(**c.kwargs(t), apply=False)
    assert got["nfused"].sum() > 50


def test_timing_reports_four_stages(gpu):
    from c_orb_slam_amd._lib import ORB_E_INVALID, OrbGpuError
    c = lc.case("stereo")
    t = c.table_copy()
    m = gpu.ORBmatcher(0.6, True)
    mp = c.fill(gpu.Map())
    lcl = gpu.LoopClosing(m, mp)
    with pytest.raises(OrbGpuError) as ei:
        lcl.last_searchandfuse_timings()
    assert ei.value.code == ORB_E_INVALID                               # before the first timed call
    mp.enable_timing(True)
    lcl.SearchAndFuse(**c.kwargs(t), apply=False)
    ms = lcl.last_searchandfuse_timings()
    print("projection, match, descriptors, host replay (ms):", ms.tolist())
    assert ms.shape == (4,) and (ms >= 0).all() and ms[1] > 0 and ms[3] > 0


def test_shuffled_keyframes_give_the_same_ops(gpu, reference):
    c = lc.case("mono")
    want = reference["mono"][1].result()
    order = [2, 0, 3, 1]
    t = c.table_copy()
    _, _, got = run_library(gpu, c, t, order=order)
    new_index = {old: new for new, old in enumerate(order)}             # pass = the index into the kf[] given
    ops = want["ops"].copy()
    for o in ops:
        if o[0] >= 0:
            o[0] = new_index[int(o[0])]
    assert same_bytes(got["ops"], ops) and same_bytes(got["nfused"], want["nfused"][order])
    assert same_bytes(got["updated"], want["updated"])
    assert_same_table(t, reference["mono"][1].t, "shuffled")
