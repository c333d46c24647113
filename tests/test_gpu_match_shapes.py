"""The guided matcher (k_build_grid, k_candidates, k_select_r, k_frustum) over frame sizes, query
counts, batch sizes and grid geometries, bit-exact against the CPU oracle.

tests/test_gpu_match.py and tests/test_gpu_track_local_map.py run extractor output at one shape
(1241 x 376, about 1,200 keypoints, up to 3 problems).  Matcher::run forks on the largest frame of
the batch (LDS-staged candidate search up to 1,536 keypoints, device-memory walk above), on the
query count (register slots up to 4,096 queries, qinfo state beyond) and on the problem count
(XCD-aware block order from 8 problems).  The problems here are synthetic (tests/match_cases.py;
tests/test_match_cases_cpu.py shows on the oracle alone that they are not vacuous), every result
is compared with np.array_equal, and ORBmatcher_last_search_plan tells which launches ran.
"""
import ctypes as C

import numpy as np
import pytest

import match_cases as mc
import oracle_lib

pytestmark = pytest.mark.gpu

LADDER = [c.id for c in mc.PAIR_CASES if "ladder" in c.tags]
GEOMETRY = [c.id for c in mc.PAIR_CASES if "geometry" in c.tags]
CROWDED = [c.id for c in mc.PAIR_CASES if "crowded" in c.tags]


@pytest.fixture(scope="module")
def m_last(gpu):
    return gpu.ORBmatcher(0.9, True)      # TrackWithMotionModel's matcher, Tracking.cc:869


@pytest.fixture(scope="module")
def m_local(gpu):
    return gpu.ORBmatcher(0.8, False)     # SearchLocalPoints' matcher, Tracking.cc:1184


def _mono(pair):
    return pair[0].uRight is None


def _oracle_last(pair, th, bMono, init=None):
    cur, last, mps, last_mp, last_outlier, lk = pair
    o = np.full(cur.N, -1, np.int32) if init is None else init.copy()
    return oracle_lib.oracle_search_last(cur, o, last, lk, last_mp, last_outlier, mps, th, bMono, 0.9, True), o


def _gpu_last(m, pair, th, bMono):
    cur, last, mps, last_mp, last_outlier, lk = pair
    g = np.full(cur.N, -1, np.int32)
    return m.SearchByProjection_LastFrame(cur, g, last, lk, last_mp, last_outlier, mps, th, bMono), g


def _check_last(m, pair, th, what):
    no, o = _oracle_last(pair, th, _mono(pair))
    ng, g = _gpu_last(m, pair, th, _mono(pair))
    assert ng == no, (what, th, ng, no)
    assert np.array_equal(g, o), (what, th, np.nonzero(g != o)[0][:10])
    return m.last_search_plan()


def _check_local(m, pair, loc, th, what, nnratio=0.8):
    cur, mps = pair[0], pair[2]
    in_view, px, pxr, py, level, view_cos, mp_index, cur_mp = loc
    g, o = cur_mp.copy(), cur_mp.copy()
    no = oracle_lib.oracle_search_local(cur, o, mps.obs, in_view, px, pxr, py, level, view_cos, mps.desc[mp_index],
                                        mp_index, th, nnratio)
    ng = m.SearchByProjection_MapPoints(cur, g, in_view, px, pxr, py, level, view_cos, mp_index, mps, th)
    assert ng == no, (what, th, ng, no)
    assert np.array_equal(g, o), (what, th, np.nonzero(g != o)[0][:10])
    return m.last_search_plan()


def _want_plan(plan, n, nq, np_, select, staged=None):
    """The launches for a batch whose largest frame has n keypoints and largest problem nq queries."""
    if staged is None:
        staged = n <= mc.STAGE_MAX_N
    want = dict(staged=int(staged and nq > 0), cand_threads=0 if nq == 0 else 1024 if staged else 256,
                select_threads=select if nq > 0 else 0, max_n=max(n, 1), max_q=nq, np=np_)
    assert plan == want, (plan, want)


@pytest.mark.parametrize("cid", LADDER)
def test_last_frame_ladder(m_last, cid):
    case, pair = mc.PAIR_BY_ID[cid], mc.pair_of(cid)
    for th in mc.LAST_TH:
        _want_plan(_check_last(m_last, pair, th, cid), case.n_cur, case.n_last, 1, 512)


@pytest.mark.parametrize("cid", LADDER)
def test_map_points_ladder(m_local, cid):
    case, pair, loc = mc.PAIR_BY_ID[cid], mc.pair_of(cid), mc.local_of(cid)
    for th in mc.LOCAL_TH:
        _want_plan(_check_local(m_local, pair, loc, th, cid), case.n_cur, case.n_last, 1, 1024)


def test_plan_of_a_fresh_matcher(gpu):
    """Before the first search there is no plan to report: ORB_E_INVALID, not zeros that read as one."""
    from c_orb_slam_amd._lib import ORB_E_INVALID
    m = gpu.ORBmatcher(0.9, True)
    with pytest.raises(gpu.OrbGpuError) as ei:
        m.last_search_plan()
    assert ei.value.code == ORB_E_INVALID
    _check_last(m, mc.pair_of("ladder-63-mono"), 15.0, "first search")
    assert m.last_search_plan()["np"] == 1


def test_no_query_count_is_zero(m_last, m_local):
    """A search without a single query launches no selection kernel; the count it would have
    written must still come back 0, whatever an earlier call left in the count's device slot."""
    busy = mc.pair_of("ladder-63-mono")
    for cid in ("last-0", "ladder-0-mono"):
        pair = mc.pair_of(cid)
        assert _gpu_last(m_last, busy, 15.0, True)[0] > 0
        assert _gpu_last(m_last, pair, 15.0, True)[0] == 0
        _check_local(m_local, busy, mc.local_of("ladder-63-mono"), 5.0, "busy")
        _check_local(m_local, pair, mc.local_of(cid), 5.0, cid)


def test_frames_above_the_limit_are_refused(gpu, m_last, m_local):
    """4,097 keypoints in the current frame (both searches) or in the last frame: ORB_E_INVALID,
    cur_mp and the count untouched."""
    from c_orb_slam_amd._lib import ORB_E_INVALID, KP_DTYPE, lib, ptr
    L = lib()
    big = mc.synth_pair(np.random.default_rng(9), 300, mc.MAX_FRAME_KEYS + 1, 640, 480)
    ok = mc.pair_of("ladder-63-mono")
    for cur, last_pair in ((big[0], ok), (ok[0], mc.synth_pair(np.random.default_rng(10), mc.MAX_FRAME_KEYS + 1, 63,
                                                               640, 480))):
        _, last, mps, last_mp, last_outlier, lk = last_pair
        g = np.full(cur.N, -5, np.int32)
        n = C.c_int(-77)
        cf, lf, mp = cur.cstruct(), last.cstruct(), mps.cstruct()
        lk = np.ascontiguousarray(lk, KP_DTYPE)
        rc = L.ORBmatcher_SearchByProjection_LastFrame(m_last._h, C.byref(cf), ptr(g), C.byref(lf), ptr(lk), ptr(last_mp),
                                                       ptr(last_outlier), C.byref(mp), 15.0, 1, C.byref(n))
        assert rc == ORB_E_INVALID and n.value == -77 and (g == -5).all()
    loc = mc.synth_local(np.random.default_rng(11), big, 200)
    g = np.full(big[0].N, -5, np.int32)
    with pytest.raises(gpu.OrbGpuError) as ei:
        m_local.SearchByProjection_MapPoints(big[0], g, *loc[:7], big[2], 1.0)
    assert ei.value.code == ORB_E_INVALID and (g == -5).all()
    _check_last(m_last, ok, 15.0, "after the refusals")     # the handle still works


@pytest.mark.parametrize("cid", GEOMETRY)
def test_grid_geometry(m_last, m_local, cid):
    """Image sizes 320 x 240, 752 x 480 and 1241 x 376 with bounds beyond the image (negative minX /
    minY): keypoints outside the bounds (cell -1) and on maxX / maxY (column 64 / row 48: dropped)."""
    case, pair = mc.PAIR_BY_ID[cid], mc.pair_of(cid)
    for th in mc.LAST_TH:
        _want_plan(_check_last(m_last, pair, th, cid), case.n_cur, case.n_last, 1, 512)
    for th in mc.LOCAL_TH:
        _check_local(m_local, pair, mc.local_of(cid), th, cid)


@pytest.mark.parametrize("th", mc.CROWDED_TH)
@pytest.mark.parametrize("cid", CROWDED)
def test_crowded_cell(m_last, cid, th):
    """60 % / all of 1,536 (staged) and 4,096 (unstaged) keypoints in one grid cell: the 16-bit packed
    counters and the stable-rank loop of k_build_grid at their top, windows far beyond kTopK (the
    rescan of select_slow), long occupancy chains (one workgroup replays them: the 4,096-keypoint
    cell takes between one and two seconds per search)."""
    case, pair = mc.PAIR_BY_ID[cid], mc.pair_of(cid)
    _want_plan(_check_last(m_last, pair, th, cid), case.n_cur, case.n_last, 1, 512)


@pytest.mark.parametrize("cid", CROWDED)
def test_crowded_cell_map_points(m_local, cid):
    case, pair = mc.PAIR_BY_ID[cid], mc.pair_of(cid)
    _want_plan(_check_local(m_local, pair, mc.local_of(cid), 5.0, cid), case.n_cur, case.n_last, 1, 1024)


@pytest.mark.parametrize("nq", mc.BEYOND_NQ)
@pytest.mark.parametrize("fid", mc.BEYOND_FRAMES)
def test_map_points_beyond_the_slots(m_local, fid, nq):
    """More queries than k_select_r's 4,096 register slots: the rest decide through select_slow with
    their state in qinfo."""
    pair = mc.pair_of(fid)
    for th in mc.LOCAL_TH:
        _want_plan(_check_local(m_local, pair, mc.beyond_local(fid, nq), th, (fid, nq)), pair[0].N, nq, 1, 1024)


@pytest.mark.parametrize("fid", ["map-1500", "map-2500"])
def test_search_local_points_beyond_the_slots(m_local, fid):
    """A local map with more than 4,600 in-view points: k_frustum's in-view list comes in any order,
    and the part of it past the register slots differs from run to run; the result must not."""
    F, cm, M = mc.big_local_map(fid)
    for th in mc.LOCAL_TH:
        o = cm.copy()
        no, nvo = oracle_lib.oracle_search_local_points(F, o, M, mc.LOG_SCALE_FACTOR, th, 0.8)
        assert nvo >= 4600
        for rep in range(2):
            g = [cm.copy()]
            nm, nv = m_local.SearchLocalPoints([F], g, [M], mc.LOG_SCALE_FACTOR, th)
            assert (nm[0], nv[0]) == (no, nvo), (th, rep)
            assert np.array_equal(g[0], o), (th, rep, np.nonzero(g[0] != o)[0][:10])
        _want_plan(m_local.last_search_plan(), F.N, len(M["pos"]), 1, 1024)


@pytest.mark.parametrize("np_", mc.BATCH_NP)
def test_last_frame_batches(m_last, np_):
    """1 to 17 problems in one launch set: below 8 the blocks are laid out problem by problem, from 8
    on XCD-aware with padding blocks when np is no multiple of 8.  Frames of 0, 1, 200 and 300
    keypoints, a problem without a query."""
    pairs = [p[0] for p in mc.batch_problems(np_)]
    outs = [np.full(p[0].N, -1, np.int32) for p in pairs]
    nm = m_last.SearchByProjection_LastFrame_batch([p[0] for p in pairs], outs, [p[1] for p in pairs],
                                                   [p[5] for p in pairs], [p[3] for p in pairs], [p[4] for p in pairs],
                                                   [p[2] for p in pairs], 15.0, False)
    _want_plan(m_last.last_search_plan(), max(p[0].N for p in pairs), max(p[1].N for p in pairs), np_, 512)
    for k, (pair, g, n) in enumerate(zip(pairs, outs, nm)):
        no, o = _oracle_last(pair, 15.0, False)
        assert n == no and np.array_equal(g, o), (k, n, no)


@pytest.mark.parametrize("np_", mc.BATCH_NP)
def test_search_local_points_batches(m_local, np_):
    """k_frustum and k_candidates<false> share the block order; here also an empty local map and one
    with no point in view."""
    probs = mc.batch_problems(np_)
    frames, maps = [p[0][0] for p in probs], [p[1] for p in probs]
    g = [p[2].copy() for p in probs]
    nm, nv = m_local.SearchLocalPoints(frames, g, maps, mc.LOG_SCALE_FACTOR, 3.0)
    _want_plan(m_local.last_search_plan(), max(F.N for F in frames), max(len(M["pos"]) for M in maps), np_, 1024)
    for k, (p, gk) in enumerate(zip(probs, g)):
        o = p[2].copy()
        no, nvo = oracle_lib.oracle_search_local_points(frames[k], o, maps[k], mc.LOG_SCALE_FACTOR, 3.0, 0.8)
        assert (nm[k], nv[k]) == (no, nvo), k
        assert np.array_equal(gk, o), (k, np.nonzero(gk != o)[0][:10])


@pytest.mark.parametrize("ids", mc.MIXED_BATCHES, ids="+".join)
def test_mixed_batches(m_last, m_local, ids):
    """The largest frame of the batch chooses the candidate path and sizes the LDS arrays of every
    problem: 300 + 1,537 and 1,536 + 1,537 keypoints run unstaged, 1,536 + 1,536 staged; each problem
    equals the oracle and its single call."""
    pairs = [mc.pair_of(i) for i in ids]
    staged = ids == ("mix-1536a", "mix-1536b")
    for th in mc.LAST_TH:
        outs = [np.full(p[0].N, -1, np.int32) for p in pairs]
        nm = m_last.SearchByProjection_LastFrame_batch([p[0] for p in pairs], outs, [p[1] for p in pairs],
                                                       [p[5] for p in pairs], [p[3] for p in pairs],
                                                       [p[4] for p in pairs], [p[2] for p in pairs], th, False)
        _want_plan(m_last.last_search_plan(), max(p[0].N for p in pairs), max(p[1].N for p in pairs), 2, 512, staged)
        for pair, g, n in zip(pairs, outs, nm):
            no, o = _oracle_last(pair, th, False)
            ns, s = _gpu_last(m_last, pair, th, False)
            assert n == no == ns and np.array_equal(g, o) and np.array_equal(g, s), (ids, th)
    maps = mc.mixed_local_maps(ids)
    frames = [p[0] for p in pairs]
    cms = [np.full(F.N, -1, np.int32) for F in frames]
    g = [c.copy() for c in cms]
    nm, nv = m_local.SearchLocalPoints(frames, g, maps, mc.LOG_SCALE_FACTOR, 1.0)
    _want_plan(m_local.last_search_plan(), max(F.N for F in frames), max(len(M["pos"]) for M in maps), 2, 1024, staged)
    for k in range(2):
        o = cms[k].copy()
        no, nvo = oracle_lib.oracle_search_local_points(frames[k], o, maps[k], mc.LOG_SCALE_FACTOR, 1.0, 0.8)
        s = [cms[k].copy()]
        ns, nvs = m_local.SearchLocalPoints([frames[k]], s, [maps[k]], mc.LOG_SCALE_FACTOR, 1.0)
        assert (nm[k], nv[k]) == (no, nvo) == (ns[0], nvs[0]) and no > 50
        assert np.array_equal(g[k], o) and np.array_equal(g[k], s[0])
