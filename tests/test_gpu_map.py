"""The device-resident Map against the literal restatement (tests/map_ref.py): every mutation, the vote,
Tracking::UpdateLocalMap and KeyFrame::UpdateConnections.  Everything is integer work: every comparison
is exact equality.  The shapes are the smallest that reach every path: a keyframe count on either side
of a workgroup multiple, rows of 64-600 slots, 500-5,000 map points, frames of at most 1,500 keypoints."""
import ctypes as C
import threading

import numpy as np
import pytest

import map_cases as mc
from c_orb_slam_amd._lib import ORB_E_CAPACITY, ORB_E_INVALID, lib, orb_localmap, orb_localprep, orb_localupdate, ptr
from map_ref import RefMap

pytestmark = pytest.mark.gpu


@pytest.fixture()
def knobs():
    """The process-wide test knobs are back at their defaults after the test."""
    L = lib()
    yield L
    L.orbgpu_unit_set_map_initial_capacity(0, 0, 0)
    L.orbgpu_unit_set_map_chunk(0)
    L.orbgpu_unit_set_map_lds_slots(-1)


class Pair:
    """A library Map and a RefMap that receive the same calls."""

    def __init__(self, gpu, n_pts):
        self.map, self.ref, self.n_pts = gpu.Map(), RefMap(), n_pts
        self.m = gpu.ORBmatcher(0.8, False)

    def apply(self, ops):
        mc.apply(self.map, ops)
        mc.apply(self.ref, ops)

    def check_frames(self, frames, m=None, **kw):
        """UpdateLocalMap of `frames` in one batch == the restatement frame by frame.  -> the results"""
        bad = self.ref.bad_flags(self.n_pts)
        cur = [f.copy() for f in frames]
        got = (m or self.m).UpdateLocalMap(self.map, cur, bad=bad, **kw)
        for f, c, g in zip(frames, cur, got):
            want_cur = [int(x) for x in f]
            want = self.ref.UpdateLocalMap(want_cur)
            assert c.tolist() == want_cur                         # bad points cleared
            if want is None:
                assert (g["n_kf"], g["ref_kf"], g["n_pt"]) == (0, -1, 0) and g["cur_row"] is None
                continue
            assert g["local_kf"].tolist() == want["local_kf"]
            assert g["ref_kf"] == want["ref_kf"]
            assert g["local_mp"].tolist() == want["local_mp"]
            assert g["cur_row"].tolist() == want["cur_row"]
        return got

    def check_connections(self, ids=None):
        ids = sorted(k for k, kf in self.ref.kfs.items() if not kf.isBad()) if ids is None else ids
        got = self.map.UpdateConnections_batch(ids)
        for k, g in zip(ids, got):
            want = self.ref.UpdateConnections(k)
            assert tuple(x.tolist() for x in g) == tuple(want), k
        return got


def build(gpu, seed, n_kf, row, n_pts, hot=0, erase=(), reuse=0, **kw):
    """A map of n_kf keyframes; `erase` ids are erased afterwards and `reuse` new keyframes added into the
    freed storage (so that slot order is no longer id order); neighbours name erased ids as well."""
    p = Pair(gpu, n_pts)
    p.apply(mc.gen_map(seed, n_kf, row, n_pts, hot=hot, **kw))
    p.apply([("EraseKeyFrame", int(k)) for k in erase])
    if reuse:
        extra = mc.gen_map(seed + 1, reuse, row, n_pts)
        # ids interleaved with and beyond the old ones
        p.apply([("AddKeyFrame", int(erase[i]) if i % 2 == 0 and i < len(erase) else n_kf + i, op[2], op[3])
                 for i, op in enumerate(extra)])
    p.apply(mc.gen_neighbours(seed + 2, p.ref, extra_ids=list(erase) + [n_kf + 1000]))
    return p


CASES = {
    # name: (n_kf, row, n_pts, hot, erase, reuse, N)
    "one_keyframe": (1, 64, 500, 0, (), 0, 100),
    "three_keyframes": (3, 64, 500, 0, (), 0, 257),
    "below_workgroup": (255, 96, 2000, 70, (), 0, 700),
    "above_workgroup": (257, 96, 2000, 70, (), 0, 700),
    "wide_rows": (40, 600, 5000, 0, (), 0, 1500),
    "slot_reuse": (60, 128, 1500, 0, (3, 10, 11, 30, 59), 5, 512),
}


@pytest.mark.parametrize("name", list(CASES))
def test_generated_case_matches_restatement(gpu, name):
    n_kf, row, n_pts, hot, erase, reuse, N = CASES[name]
    p = build(gpu, len(name), n_kf, row, n_pts, hot=hot, erase=erase, reuse=reuse)
    frames = mc.gen_frames(7, p.ref, 4, N, n_pts)
    frames.append(np.full(N, -1, np.int32))                               # an empty vote
    if hot:
        frames.append(np.array([0, 0, 5, -1], np.int32))                  # the hot point, twice
    got = p.check_frames(frames, kf_cap=max(n_kf + reuse, 4), pt_cap=n_pts)
    p.check_connections()
    if hot:
        assert len(p.ref.pts[0].mObservations) > 64 and got[-1]["n_kf"] > 50
    assert got[0]["n_kf"] > 0 and got[-2 if hot else -1]["n_kf"] == 0


def test_more_than_80_voted_keyframes(gpu):
    p = build(gpu, 5, 120, 64, 800, hot=100, p_unobserved=0.0)
    g = p.check_frames([np.array([0, -1, 0], np.int32)], kf_cap=200, pt_cap=800)
    assert g[0]["local_kf"].tolist() == list(range(100))                  # nothing is appended
    # exactly 80 voted: one more iteration runs, and it appends something
    p2 = build(gpu, 6, 120, 64, 800, hot=80, p_unobserved=0.0)
    g = p2.check_frames([np.array([0], np.int32)], kf_cap=200, pt_cap=800)
    assert g[0]["local_kf"].tolist()[:80] == list(range(80)) and 80 < g[0]["n_kf"] <= 83


def test_known_answers_on_the_device(gpu):
    """The hand-computed answers of test_map_cpu.py, asked of the library."""
    p = Pair(gpu, 64)
    p.apply([("AddKeyFrame", 1, np.array([0], np.int32), None), ("AddKeyFrame", 2, np.array([1], np.int32), None),
             ("AddKeyFrame", 10, np.array([7], np.int32), None), ("AddKeyFrame", 11, np.array([8], np.int32), None),
             ("SetNeighbours", 1, [], 10, []), ("SetNeighbours", 2, [11], -1, [])])
    g = p.m.UpdateLocalMap(p.map, [np.array([0, 1], np.int32)])[0]
    assert g["local_kf"].tolist() == [1, 2, 10] and g["ref_kf"] == 1 and g["local_mp"].tolist() == [0, 1, 7]
    q = Pair(gpu, 64)
    q.apply([("AddKeyFrame", 1, np.array([0, 1], np.int32), np.array([1, 0], np.uint8)),
             ("AddKeyFrame", 2, np.array([1], np.int32), None)])
    assert q.m.UpdateLocalMap(q.map, [np.array([1], np.int32)])[0]["local_kf"].tolist() == [2]
    g = q.m.UpdateLocalMap(q.map, [np.array([0], np.int32)])[0]
    assert g["local_kf"].tolist() == [1] and g["local_mp"].tolist() == [0, 1]
    pts = np.arange(16, dtype=np.int32)
    r = Pair(gpu, 64)
    r.apply([("AddKeyFrame", k, pts, None) for k in (1, 2, 4)])
    cid, cn, oid, ow = r.map.UpdateConnections(1)
    assert (cid.tolist(), cn.tolist(), oid.tolist(), ow.tolist()) == ([2, 4], [16, 16], [4, 2], [16, 16])
    # duplicate id, and a point that a sparse update would put into a row twice
    L = lib()
    assert L.Map_AddKeyFrame(r.map._h, 2, 16, ptr(pts), None) == ORB_E_INVALID
    assert L.Map_SetMapPointMatches(r.map._h, 2, 1, ptr(np.array([3], np.int32)), ptr(np.array([5], np.int32)),
                                    None) == ORB_E_INVALID
    assert L.Map_SetNeighbours(r.map._h, 99, 0, None, -1, 0, None) == ORB_E_INVALID
    assert r.map.size() == (3, 48, 48)


def test_mutate_then_query(gpu, knobs):
    """Each mutation entry, then a query, equals the restatement after the same mutation; the handle starts
    with room for 4 keyframes, 256 slots and 64 point ids, so every pool grows on the way."""
    knobs.orbgpu_unit_set_map_initial_capacity(4, 256, 64)
    n_pts = 1200
    p = build(gpu, 11, 30, 96, n_pts)
    frames = mc.gen_frames(3, p.ref, 3, 400, n_pts)
    caps = dict(kf_cap=64, pt_cap=n_pts)
    p.check_frames(frames, **caps)
    rng = np.random.default_rng(0)
    rows = {k: [m.mnId if m else -1 for m in kf.mvpMapPoints] for k, kf in p.ref.kfs.items()}
    # SetMapPointMatches: erase, add unobserved, add observed, flip an observation, move within the row
    r7 = rows[7]
    held = [i for i, v in enumerate(r7) if v >= 0]
    free = [i for i, v in enumerate(r7) if v < 0]
    p.apply([("SetMapPointMatches", 7, np.array(held[:3], np.int32), np.array([-1, -1, -1], np.int32), None),
             ("SetMapPointMatches", 7, np.array(free[:2], np.int32), np.array([1100, 1101], np.int32),
              np.array([0, 1], np.uint8)),
             ("SetMapPointMatches", 7, np.array([held[4]], np.int32), np.array([r7[held[4]]], np.int32),
              np.array([0], np.uint8)),
             ("SetMapPointMatches", 7, np.array([held[5], free[3]], np.int32), np.array([-1, r7[held[5]]], np.int32),
              None)])
    p.check_frames(frames + [np.array([1100, 1101, r7[held[4]]], np.int32)], **caps)
    p.check_connections([7, 8])
    # EraseMapPoint of observed points; ReplaceMapPoint hitting both branches
    seen = lambda k: {q for q, m in p.ref.pts.items() if p.ref.kfs[k] in m.mObservations}
    both = sorted(seen(12) & seen(13))
    only12 = [a for a in rows[12] if a >= 0 and a not in rows[13]]
    assert len(both) >= 2 and only12
    p.apply([("EraseMapPoint", both[0])])
    # rows 12 and 13 both hold both[1]; only row 12 holds only12[0]: in row 12 the slot is emptied (the
    # row already holds the replacement), in row 13 it takes it
    p.apply([("ReplaceMapPoint", both[1], only12[0])])
    assert only12[0] in [m.mnId for m in p.ref.kfs[13].mvpMapPoints if m]
    assert both[1] not in [m.mnId for m in p.ref.kfs[12].mvpMapPoints if m]
    p.check_frames(frames + [np.array([both[0], both[1], only12[0]], np.int32)], **caps)
    p.check_connections([12, 13])
    # EraseKeyFrame, a new keyframe in its place, new neighbours
    p.apply([("EraseKeyFrame", 12), ("AddKeyFrame", 40, np.array(rows[5][:64], np.int32), None)])
    p.apply(mc.gen_neighbours(9, p.ref, extra_ids=[12]))
    p.check_frames(frames, **caps)
    p.check_connections()
    n_kf, n_slots, n_obs = p.map.size()
    assert n_kf == 30 and n_slots == 29 * 96 + 64
    assert n_obs == sum(len(m.mObservations) for m in p.ref.pts.values())
    p.map.clear()
    assert p.map.size() == (0, 0, 0)
    assert p.m.UpdateLocalMap(p.map, [frames[0].copy()])[0]["n_kf"] == 0


def test_batch_chunks_and_counter_placement(gpu, knobs):
    """A batch equals single calls for batches of 1, 3 and one more than the chunk size; counters in LDS
    equal counters in device memory."""
    n_pts = 1500
    p = build(gpu, 21, 70, 128, n_pts)
    frames = mc.gen_frames(5, p.ref, 5, 600, n_pts)
    caps = dict(kf_cap=128, pt_cap=n_pts)
    single = [p.check_frames([f], **caps)[0] for f in frames]
    knobs.orbgpu_unit_set_map_chunk(4)
    for nb in (1, 3, 5):
        for lds in (-1, 0):
            knobs.orbgpu_unit_set_map_lds_slots(lds)
            got = p.check_frames(frames[:nb], **caps)
            for g, s in zip(got, single):
                assert all(np.array_equal(g[k], s[k]) for k in ("local_kf", "local_mp", "cur_row"))
            conn = p.check_connections()
    knobs.orbgpu_unit_set_map_lds_slots(-1)
    knobs.orbgpu_unit_set_map_chunk(0)
    ref_conn = p.check_connections()
    assert all(np.array_equal(a, b) for x, y in zip(conn, ref_conn) for a, b in zip(x, y))


def test_capacity_is_reported_and_nothing_written_past_it(gpu):
    n_pts = 1000
    p = build(gpu, 31, 40, 96, n_pts)
    f = mc.gen_frames(2, p.ref, 1, 300, n_pts)[0]
    full = p.check_frames([f], kf_cap=64, pt_cap=n_pts)[0]
    n_kf, n_pt = full["n_kf"], full["n_pt"]
    assert n_kf > 2 and n_pt > 2
    L = lib()
    for kc, pc in ((n_kf - 1, n_pt), (n_kf, n_pt - 1)):
        kf = np.full(n_kf + 4, -77, np.int32)
        lp = np.full(n_pt + 4, -77, np.int32)
        cur, row = f.copy(), np.full(len(f), -77, np.int32)
        u = orb_localupdate()
        u.N, u.cur_mp, u.kf_cap, u.pt_cap = len(f), ptr(cur), kc, pc
        u.local_kf, u.local_mp, u.cur_row = ptr(kf), ptr(lp), ptr(row)
        assert L.ORBmatcher_set_device_pointers(p.m._h, 0) == 0
        assert L.Tracking_UpdateLocalMap_batch(p.m._h, p.map._h, 1, C.byref(u)) == ORB_E_CAPACITY
        assert (u.n_kf, u.n_pt) == (n_kf, n_pt)
        assert np.all(kf[kc:] == -77) and np.all(lp[pc:] == -77)
        assert np.array_equal(kf[:kc], full["local_kf"][:kc]) and np.array_equal(lp[:pc], full["local_mp"][:pc])
        u.kf_cap, u.pt_cap = u.n_kf, u.n_pt                                   # the retry
        assert L.Tracking_UpdateLocalMap_batch(p.m._h, p.map._h, 1, C.byref(u)) == 0
        assert np.array_equal(kf[:n_kf], full["local_kf"]) and np.array_equal(lp[:n_pt], full["local_mp"])
        assert np.all(kf[n_kf:] == -77) and np.all(lp[n_pt:] == -77)
        assert np.array_equal(row, full["cur_row"])
    # the Python wrapper retries by itself; UpdateConnections reports its counts the same way
    g = p.m.UpdateLocalMap(p.map, [f.copy()], kf_cap=1, pt_cap=1)[0]
    assert np.array_equal(g["local_mp"], full["local_mp"])
    want = p.ref.UpdateConnections(5)
    got = p.map.UpdateConnections_batch([5], cap_counter=1, cap_ordered=1)[0]
    assert tuple(x.tolist() for x in got) == tuple(want) and len(want[0]) > 1


def test_two_host_threads_query_one_handle(gpu):
    """Two host threads, each with its own matcher (its own stream), query one Map right after a mutation:
    one of them rebuilds the index, the other waits for it on the device; both equal the sequential answers."""
    n_pts = 1500
    p = build(gpu, 41, 70, 128, n_pts)
    frames = mc.gen_frames(8, p.ref, 6, 500, n_pts)
    caps = dict(kf_cap=128, pt_cap=n_pts)
    want = p.check_frames(frames, **caps)
    p.apply([("SetMapPointMatches", 3, np.array([0], np.int32), np.array([-1], np.int32), None)])
    want = p.check_frames(frames, **caps)
    p.apply([("SetMapPointMatches", 4, np.array([0], np.int32), np.array([-1], np.int32), None)])   # dirty again
    want2 = [p.ref.UpdateLocalMap([int(x) for x in f]) for f in frames]
    ms = [gpu.ORBmatcher(0.8, False), gpu.ORBmatcher(0.8, False)]
    out, err = [None, None], []

    def work(t):
        try:
            out[t] = ms[t].UpdateLocalMap(p.map, [f.copy() for f in frames[t::2]], **caps)
        except Exception as e:   # noqa: BLE001
            err.append(e)

    th = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=60)
    assert not err and not any(t.is_alive() for t in th)
    for t in range(2):
        for g, w in zip(out[t], want2[t::2]):
            assert g["local_kf"].tolist() == w["local_kf"] and g["local_mp"].tolist() == w["local_mp"]
            assert g["cur_row"].tolist() == w["cur_row"] and g["ref_kf"] == w["ref_kf"]
    del want


# ---------------------------------------------------------------- the deferred chain

def _device_update(gpu, m, mp, frames_mp, table, kf_cap, pt_cap, deferred, dev):
    """Tracking_UpdateLocalMap_batch with device pointers and the gather.  -> (structs, tensors).  The
    synchronous form gathers the descriptors into rows one byte off a 16-byte boundary."""
    import torch
    off = 0 if deferred else 1
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    n = len(table["pos"])
    T = dict(pos=t(table["pos"]), desc=t(table["desc"]), obs=t(table["obs"]), mx=t(table["max_dist"]),
             mn=t(table["min_dist"]), nrm=t(table["normal"]), bad=t(table["bad"]))
    tab = orb_localmap(n, T["pos"].data_ptr(), T["desc"].data_ptr(), T["obs"].data_ptr(), T["mx"].data_ptr(),
                       T["mn"].data_ptr(), T["nrm"].data_ptr(), T["bad"].data_ptr())
    ua = (orb_localupdate * len(frames_mp))()
    outs = []
    for u, f in zip(ua, frames_mp):
        z = lambda shape, dt: torch.full(shape, 9, dtype=dt, device=dev)
        o = dict(cur=t(f), kf=z((kf_cap,), torch.int32), lp=z((pt_cap,), torch.int32), crow=z((len(f),), torch.int32),
                 row=z((pt_cap,), torch.int32), pos=z((pt_cap, 3), torch.float32),
                 desc=z((pt_cap * 32 + 16,), torch.uint8)[off:off + pt_cap * 32].view(pt_cap, 32),
                 obs=z((pt_cap,), torch.int32), mx=z((pt_cap,), torch.float32), mn=z((pt_cap,), torch.float32),
                 nrm=z((pt_cap, 3), torch.float32), skip=z((pt_cap,), torch.uint8))
        u.N, u.cur_mp, u.table, u.kf_cap, u.pt_cap = len(f), o["cur"].data_ptr(), C.pointer(tab), kf_cap, pt_cap
        u.local_kf, u.local_mp, u.cur_row, u.row = (o[k].data_ptr() for k in ("kf", "lp", "crow", "row"))
        u.pos, u.desc, u.observations, u.max_dist, u.min_dist, u.normal, u.skip = (
            o[k].data_ptr() for k in ("pos", "desc", "obs", "mx", "mn", "nrm", "skip"))
        outs.append(o)
    return ua, outs, (T, tab)


def test_deferred_chain_equals_synchronous_and_host_built_local_map(gpu):
    """UpdateLocalMap -> PrepareLocalSearch -> SearchLocalPoints as one deferred chain gives the matches and
    counts of the same two calls fed a local map built on the host from the restatement's lists; and the
    deferred UpdateLocalMap equals the synchronous one bit for bit."""
    import torch
    from c_orb_slam_amd import synthetic
    from match_cases import local_map
    from test_gpu_track_local_map import H, W, cur_frame
    dev = torch.device("cuda", 0)
    L = lib()
    frames_img, Hs, Rs = synthetic.sequence(33, 3, return_rotations=True)
    ex = gpu.ORBextractor(1200, 1.2, 8, 20, 7, max_width=W, max_height=H, max_batch=3)
    res = ex.extract_batch(frames_img)
    scale = ex.GetScaleFactors()
    lsf = np.float32(np.log(np.float32(1.2)))
    rng = np.random.default_rng(4)
    (k0, d0) = res[0]
    table = local_map(rng, k0, d0, scale)                                   # the global map-point table
    n = len(table["pos"])
    table["bad"] = (rng.random(n) < 0.03).astype(np.uint8)
    # a map of 12 keyframes over the table; every keyframe sees a random third of it
    p = Pair(gpu, n)
    ops = []
    for k in range(12):
        mp = np.where(rng.random(600) < 0.9, rng.permutation(n)[:600], -1).astype(np.int32)
        ops.append(("AddKeyFrame", k, mp, (rng.random(600) < 0.95).astype(np.uint8)))
    p.apply(ops)
    for q in np.nonzero(table["bad"])[0][::2]:                               # half of the bad points are erased too
        p.apply([("EraseMapPoint", int(q))])
    for q in np.nonzero(table["bad"])[0][1::2]:
        p.ref.point(int(q)).mbBad = True
    p.apply(mc.gen_neighbours(1, p.ref))
    F = [cur_frame(rng, res[f + 1][0], res[f + 1][1], scale, Rs[f]) for f in range(2)]
    cur = [np.where(rng.random(f.N) < 0.15, rng.integers(0, n, f.N), -1).astype(np.int32) for f in F]
    outl = [(rng.random(f.N) < 0.1).astype(np.uint8) for f in F]
    kf_cap, pt_cap = 16, n
    m = gpu.ORBmatcher(0.8, False)
    assert L.ORBmatcher_set_device_pointers(m._h, 1) == 0
    try:
        # synchronous
        ua, so, keep_s = _device_update(gpu, m, p.map, cur, table, kf_cap, pt_cap, False, dev)
        assert L.Tracking_UpdateLocalMap_batch(m._h, p.map._h, len(F), ua) == 0
        sync_counts = [(u.n_kf, u.ref_kf, u.n_pt) for u in ua]
        # deferred: the whole chain, counts at finish
        ud, do, keep_d = _device_update(gpu, m, p.map, cur, table, kf_cap, pt_cap, True, dev)
        keep, fa, _ = m._local_batch(F, [table] * len(F), dev)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        d_out = [t(o) for o in outl]
        prep = (orb_localprep * len(F))(*[orb_localprep(f.N, o["crow"].data_ptr(), d.data_ptr(), pt_cap,
                                                        o["row"].data_ptr(), o["skip"].data_ptr())
                                          for f, o, d in zip(F, do, d_out)])
        maps = (orb_localmap * len(F))(*[orb_localmap(pt_cap, o["pos"].data_ptr(), o["desc"].data_ptr(),
                                                      o["obs"].data_ptr(), o["mx"].data_ptr(), o["mn"].data_ptr(),
                                                      o["nrm"].data_ptr(), o["skip"].data_ptr()) for o in do])
        cm = (C.c_void_p * len(F))(*[o["crow"].data_ptr() for o in do])
        nm, nv = np.zeros(len(F), np.int32), np.zeros(len(F), np.int32)
        assert L.ORBmatcher_set_deferred(m._h, 1) == 0
        assert L.Tracking_UpdateLocalMap_batch(m._h, p.map._h, len(F), ud) == 0
        assert L.Tracking_PrepareLocalSearch_batch_device(m._h, len(F), prep) == 0
        assert L.ORBmatcher_SearchLocalPoints_batch(m._h, len(F), fa, cm, maps, float(lsf), 1.0, 0.8, ptr(nm),
                                                    ptr(nv)) == 0
        assert L.ORBmatcher_finish(m._h) == 0
        assert L.ORBmatcher_set_deferred(m._h, 0) == 0
    finally:
        L.ORBmatcher_set_device_pointers(m._h, 0)
    torch.cuda.synchronize()
    assert [(u.n_kf, u.ref_kf, u.n_pt) for u in ud] == sync_counts
    for f in range(len(F)):
        want_cur = [int(x) for x in cur[f]]
        want = p.ref.UpdateLocalMap(want_cur)
        n_kf, ref_kf, n_pt = sync_counts[f]
        assert n_kf == len(want["local_kf"]) and n_pt == len(want["local_mp"]) and ref_kf == want["ref_kf"]
        for o in (so[f], do[f]):
            assert o["kf"].cpu().numpy()[:n_kf].tolist() == want["local_kf"]
            assert o["lp"].cpu().numpy()[:n_pt].tolist() == want["local_mp"]
            assert o["cur"].cpu().numpy().tolist() == want_cur
        lp = np.array(want["local_mp"])
        s = so[f]
        assert s["crow"].cpu().numpy().tolist() == want["cur_row"]
        assert np.array_equal(s["row"].cpu().numpy(), np.concatenate([lp, np.full(pt_cap - n_pt, -1)]))
        assert np.array_equal(s["skip"].cpu().numpy(), np.concatenate([np.zeros(n_pt), np.ones(pt_cap - n_pt)]))
        for key, src in (("pos", "pos"), ("desc", "desc"), ("obs", "obs"), ("mx", "max_dist"), ("mn", "min_dist"),
                         ("nrm", "normal")):
            assert np.array_equal(s[key].cpu().numpy()[:n_pt], np.asarray(table[src])[lp]), key
        assert np.array_equal(do[f]["desc"].cpu().numpy()[:n_pt], np.asarray(table["desc"])[lp])   # aligned rows
        # the host-built local map of the same frame through the same two calls
        M = {k: np.asarray(table[k])[lp] for k in ("pos", "desc", "obs", "max_dist", "min_dist", "normal")}
        crow = np.array(want["cur_row"], np.int32)
        skip = np.zeros(n_pt, np.uint8)
        skip[crow[crow >= 0]] = 1
        crow[outl[f] == 1] = -1
        M["skip"] = skip
        hn, hv = m.SearchLocalPoints([F[f]], [crow], [M], lsf, 1.0, nnratio=0.8)
        assert (int(nm[f]), int(nv[f])) == (int(hn[0]), int(hv[0])) and hn[0] > 20
        assert np.array_equal(do[f]["crow"].cpu().numpy(), crow)
    del keep, keep_s, keep_d


def test_timings_are_reported_when_enabled(gpu):
    n_pts = 800
    p = build(gpu, 51, 20, 64, n_pts)
    f = mc.gen_frames(1, p.ref, 2, 200, n_pts)
    p.map.enable_timing(True)
    p.check_frames(f, kf_cap=32, pt_cap=n_pts)
    ms = p.map.last_timings()
    assert ms[0] > 0 and np.all(ms[1:] >= 0) and ms[1:].sum() > 0
    p.check_frames(f, kf_cap=32, pt_cap=n_pts)
    assert p.map.last_timings()[0] == -1          # nothing had changed: no rebuild
    p.map.enable_timing(False)
