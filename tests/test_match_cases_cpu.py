"""CPU: the matcher's shape matrix (tests/match_cases.py) is not vacuous.

Every assertion here is a property of the CPU oracle and of numpy alone, for the very problems
tests/test_gpu_match_shapes.py and tests/test_gpu_match_paths.py run on the device: a GPU test that
compares with the oracle proves little if the oracle matches nothing, if the window never holds a
second candidate, or if no query lies past the register slots.

* match count: the oracle matches at least 30 % of the queries that have a map point (cases with
  50 queries or more; for MapPoints the in-view queries).  Only where the queries outnumber the
  frame's keypoints several times (4,096 to 9,000 queries drawn with repetition over 300 to 2,500
  keypoints, where 30 % of the queries is more than the frame can hold) the count is of the distinct
  in-view map points queried; the big local maps (4,700 in-view points over 1,500 and 2,500
  keypoints) are held to 30 % of the smaller of in-view points and free keypoints;
* forward / backward: the stereo rungs built to move by 1.5 baselines have bForward / bBackward
  set, every other case neither, and the one-sided level range changes the oracle's result;
* window and ratio matter: in the contended cases th 7 and th 15 (LastFrame), th 1 and th 5, and
  nnratio 0.6 and 0.9 (MapPoints, at th 5: at th 1 the windows of these frames rarely hold two
  keypoints of one level) give different results;
* the rotation check removes matches;
* brute-force windows (numpy, the reference's radius and level tests): in the clustered cases at
  least 20 queries see more than kTopK = 8 candidates; in the contended cases at least 20 current
  keypoints are the nearest-descriptor candidate of two or more queries ("contended" needs room
  for 20 such keypoints: the cases with 1,000 queries or more, 200 of them duplicates);
* beyond the slots: at least 50 matches of the oracle come from queries with index >= 4096
  (entries that differ from the result of the first 4,096 queries alone, so presets and earlier
  matches do not count).  nq = 4097 has one such query: there that one query must match;
* SearchLocalPoints past the slots: isInFrustum leaves at least 4,600 points in view;
* edge keypoints: at least 10 outside the bounds and one exactly on each bound.
"""
import numpy as np
import pytest

import match_cases as mc
import match_path_worker as worker
import oracle_lib

IDS = [c.id for c in mc.PAIR_CASES]


def _mono(case):
    return not case.kw.get("stereo", False)


def _last(case, th, checkOri=True):
    cur, last, mps, last_mp, last_outlier, lk = mc.pair_of(case.id)
    o = np.full(cur.N, -1, np.int32)
    n = oracle_lib.oracle_search_last(cur, o, last, lk, last_mp, last_outlier, mps, th, _mono(case), 0.9, checkOri)
    return n, o


def _local(pair, loc, th, nnratio=0.8, nq=None):
    cur, mps = pair[0], pair[2]
    in_view, px, pxr, py, level, view_cos, mp_index, cur_mp = loc
    s = slice(0, nq)
    o = cur_mp.copy()
    n = oracle_lib.oracle_search_local(cur, o, mps.obs, in_view[s], px[s], pxr[s], py[s], level[s], view_cos[s],
                                       mps.desc[mp_index[s]], mp_index[s], th, nnratio)
    return n, o


@pytest.mark.parametrize("cid", IDS)
def test_last_frame_cases(cid):
    case = mc.PAIR_BY_ID[cid]
    cur, last, mps, last_mp, last_outlier, lk = mc.pair_of(cid)
    assert cur.N == case.n_cur and last.N == case.n_last and cur.N <= mc.MAX_FRAME_KEYS
    tz = case.kw.get("tz", 0.0)
    assert mc.motion_of(mc.pair_of(cid), _mono(case)) == (tz > 0, tz < 0)
    ths = mc.CROWDED_TH if "crowded" in case.tags else mc.LAST_TH
    nq = int(((last_mp >= 0) & (last_outlier == 0)).sum())
    res = {th: _last(case, th) for th in ths}
    if nq >= 50:
        for th, (n, o) in res.items():
            assert n >= 0.3 * nq, (th, n, nq)
            assert _last(case, th, checkOri=False)[0] > n, th
    if "contended" in case.tags:
        assert not np.array_equal(res[7.0][1], res[15.0][1])
        q, mask = mc.last_windows(mc.pair_of(cid), 15.0, _mono(case))
        assert mc.contended_keypoints(mps.desc[last_mp[q]], cur.desc, mask) >= 20
    if "clustered" in case.tags:
        for th in ths:
            q, mask = mc.last_windows(mc.pair_of(cid), th, _mono(case))
            assert int((mask.sum(1) > 8).sum()) >= 20, th
    if "edge" in case.tags:
        k = cur.keysUn
        outside = (k["x"] < cur.minX) | (k["x"] > cur.maxX) | (k["y"] < cur.minY) | (k["y"] > cur.maxY)
        assert int(outside.sum()) >= 10
        assert (k["x"] == cur.minX).any() and (k["x"] == cur.maxX).any()
        assert (k["y"] == cur.minY).any() and (k["y"] == cur.maxY).any()
        g = mc._in_grid(cur)      # roundf gives column 64 / row 48 on maxX / maxY (dropped), 0 on minX / minY (kept)
        assert not g[(k["x"] == cur.maxX) | (k["y"] == cur.maxY)].any() and g[k["x"] == cur.minX].all()
        assert int((~g & outside).sum()) >= 10


def test_forward_and_backward_rungs():
    """The matrix holds forward and backward stereo searches, and the one-sided level ranges
    (ORBmatcher.cc:1397-1402) give another result than the +-1 range of the same problem."""
    moving = [c for c in mc.PAIR_CASES if c.kw.get("tz", 0.0) != 0.0]
    motions = {mc.motion_of(mc.pair_of(c.id), False) for c in moving}
    assert motions == {(True, False), (False, True)}
    assert {c.n_cur for c in moving} >= {1535, 1537, 2000, 4096}     # staged and unstaged, both directions
    for c in moving:
        cur, last, mps, last_mp, last_outlier, lk = mc.pair_of(c.id)
        one_sided, both = np.full(cur.N, -1, np.int32), np.full(cur.N, -1, np.int32)
        oracle_lib.oracle_search_last(cur, one_sided, last, lk, last_mp, last_outlier, mps, 15.0, False, 0.9, True)
        oracle_lib.oracle_search_last(cur, both, last, lk, last_mp, last_outlier, mps, 15.0, True, 0.9, True)
        assert int((one_sided != both).sum()) >= 20, c.id


def _distinct_in_view(loc):
    return len(np.unique(loc[6][loc[0] != 0]))


@pytest.mark.parametrize("cid", IDS)
def test_map_points_cases(cid):
    case = mc.PAIR_BY_ID[cid]
    pair, loc = mc.pair_of(cid), mc.local_of(cid)
    assert len(loc[0]) == case.n_last
    res = {th: _local(pair, loc, th) for th in mc.LOCAL_TH}
    if len(loc[0]) >= 50:
        for th, (n, o) in res.items():
            assert n >= 0.3 * int(loc[0].sum()), (th, n, int(loc[0].sum()))
    if "contended" in case.tags:
        assert not np.array_equal(res[1.0][1], res[5.0][1])
        assert not np.array_equal(_local(pair, loc, 5.0, 0.6)[1], _local(pair, loc, 5.0, 0.9)[1])
        q, mask = mc.local_windows(pair, loc, 5.0)
        assert mc.contended_keypoints(pair[2].desc[loc[6][q]], pair[0].desc, mask) >= 20


@pytest.mark.parametrize("nq", mc.BEYOND_NQ)
@pytest.mark.parametrize("fid", mc.BEYOND_FRAMES)
def test_beyond_slot_cases(fid, nq):
    pair, loc = mc.pair_of(fid), mc.beyond_local(fid, nq)
    assert len(loc[0]) == nq
    for th in mc.LOCAL_TH:
        n, o = _local(pair, loc, th)
        assert n >= 0.3 * _distinct_in_view(loc), (th, n)
        n0, o0 = _local(pair, loc, th, nq=mc.SLOT_QUERIES)
        late = int((o != o0).sum())
        print(f"{fid} nq {nq} th {th}: {n} matches, {late} from queries past the slots")
        if nq - mc.SLOT_QUERIES > 1:
            assert late >= 50, (th, late)
        elif nq - mc.SLOT_QUERIES == 1:
            assert late == 1 and n == n0 + 1, (th, late)
        else:
            assert late == 0


def test_path_worker_cases():
    """The case list of tests/match_path_worker.py: LastFrame at th 15, MapPoints at th 5 with 200
    queries and with 4,700 over a 300-keypoint frame (604 past the slots), the batch of 9."""
    for cid in worker.LAST_CASES:
        cur, last, mps, last_mp, last_outlier, lk = mc.pair_of(cid)
        o = np.full(cur.N, -1, np.int32)
        n = oracle_lib.oracle_search_last(cur, o, last, lk, last_mp, last_outlier, mps, 15.0, True, 0.9, True)
        assert n >= 0.3 * int(((last_mp >= 0) & (last_outlier == 0)).sum())
    for cid, nq in worker.LOCAL_CASES:
        pair, loc = mc.pair_of(cid), worker.local_queries(cid, nq)
        n, o = _local(pair, loc, 5.0)
        if nq <= mc.SLOT_QUERIES:
            assert n >= 0.3 * int(loc[0].sum()), (cid, nq, n)
        else:
            assert n >= 0.3 * _distinct_in_view(loc), (cid, nq, n)
            assert int((o != _local(pair, loc, 5.0, nq=mc.SLOT_QUERIES)[1]).sum()) >= 50
    assert worker.BATCH_NP in mc.BATCH_NP      # test_batch_cases holds the batch's preconditions


@pytest.mark.parametrize("fid", ["map-1500", "map-2500"])
def test_big_local_map_cases(fid):
    F, cm, M = mc.big_local_map(fid)
    fr = oracle_lib.oracle_is_in_frustum(F, M, mc.LOG_SCALE_FACTOR)
    assert fr["nvisible"] >= 4600, fr["nvisible"]
    res = {}
    for th in mc.LOCAL_TH:
        o = cm.copy()
        res[th] = oracle_lib.oracle_search_local_points(F, o, M, mc.LOG_SCALE_FACTOR, th, 0.8)[0], o
        assert res[th][0] >= 0.3 * min(fr["nvisible"], int((cm < 0).sum())), res[th][0]
    assert not np.array_equal(res[1.0][1], res[5.0][1])


@pytest.mark.parametrize("np_", mc.BATCH_NP)
def test_batch_cases(np_):
    probs = mc.batch_problems(np_)
    assert len(probs) == np_
    sizes = {p[0][0].N for p in probs}
    assert sizes == set((300, 0, 1, 200)[:min(np_, 4)])
    nm, nv = [], []
    for pair, M, cm in probs:
        cur, last, mps, last_mp, last_outlier, lk = pair
        o = np.full(cur.N, -1, np.int32)
        nm.append(oracle_lib.oracle_search_last(cur, o, last, lk, last_mp, last_outlier, mps, 15.0, False, 0.9, True))
        oc = cm.copy()
        nv.append(oracle_lib.oracle_search_local_points(cur, oc, M, mc.LOG_SCALE_FACTOR, 3.0, 0.8))
    assert nm[0] >= 50 and nv[0][0] >= 50 and nv[0][1] >= 100
    if np_ >= 4:
        assert probs[2][0][1].N == 0 and len(probs[2][1]["pos"]) == 0           # no query
        assert len(probs[3][1]["pos"]) > 0 and nv[3] == (0, 0)                  # no in-view point
        assert len({len(p[1]["pos"]) for p in probs}) == np_                     # all query counts differ
    if np_ >= 8:
        assert sum(n > 0 for n in nm) >= np_ // 4 and sum(v[0] > 0 for v in nv) >= np_ // 4


@pytest.mark.parametrize("ids", mc.MIXED_BATCHES)
def test_mixed_batch_cases(ids):
    ns = [mc.pair_of(i)[0].N for i in ids]
    assert ns == [int(i.split("-")[1].rstrip("ab")) for i in ids]
    assert (max(ns) <= mc.STAGE_MAX_N) == (ids == ("mix-1536a", "mix-1536b"))
    for i in ids:
        cur, last, mps, last_mp, last_outlier, lk = mc.pair_of(i)
        o = np.full(cur.N, -1, np.int32)
        n = oracle_lib.oracle_search_last(cur, o, last, lk, last_mp, last_outlier, mps, 15.0, False, 0.9, True)
        assert n >= 0.3 * int(((last_mp >= 0) & (last_outlier == 0)).sum())
    for i, M in zip(ids, mc.mixed_local_maps(ids)):      # the SearchLocalPoints half, th 1
        F = mc.pair_of(i)[0]
        o = np.full(F.N, -1, np.int32)
        n, nv = oracle_lib.oracle_search_local_points(F, o, M, mc.LOG_SCALE_FACTOR, 1.0, 0.8)
        print(f"{i}: {n} matches of {nv} in-view points")
        assert nv >= 50 and n >= 0.3 * nv, (i, n, nv)
