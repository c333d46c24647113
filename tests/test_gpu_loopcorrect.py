"""LoopClosing_CorrectLoop and LoopClosing_ApplyGlobalBA against the restatement (tests/loopcorrect_ref.py)
over the cases of loopcorrect_cases.py, in both pointer spaces.  Every float result is one IEEE +, -, *, /
or sqrt sequence in a stated order (the build has contraction off and correctly rounded f32 divide and
sqrt), so poses, positions, normals and distances are compared bit for bit, the Sim3 outputs as doubles,
and the integer results and counts for equality.  The restatement of every case is computed once."""
import numpy as np
import pytest

import loopcorrect_cases as lc
from c_orb_slam_amd._lib import ORB_E_INVALID, OrbGpuError, lib

pytestmark = pytest.mark.gpu

CORRECT = lc.correct_cases()
GBA = lc.gba_cases()
SPACES = ["host", "device"]


@pytest.fixture(scope="module")
def want_correct():
    return {name: c.restate() for name, c in CORRECT.items()}


@pytest.fixture(scope="module")
def want_gba():
    return {name: c.restate() for name, c in GBA.items()}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 1: np.uint8}[a.dtype.itemsize])


def same_bits(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    bad = np.nonzero(bits(got).ravel() != bits(want).ravel())[0]
    assert bad.size == 0, (what, bad[:8].tolist(), got.ravel()[bad[:4]].tolist(), want.ravel()[bad[:4]].tolist())


class Tables:
    """The arrays of one call as numpy arrays or torch device tensors."""

    def __init__(self, space, **arrays):
        self.space = space
        if space == "device":
            import torch
            self.a = {k: (None if v is None else torch.from_numpy(np.ascontiguousarray(v)).cuda())
                      for k, v in arrays.items()}
        else:
            self.a = {k: (None if v is None else np.ascontiguousarray(v).copy()) for k, v in arrays.items()}

    def __getitem__(self, k):
        return self.a[k]

    def host(self, k):
        v = self.a[k]
        return v.cpu().numpy() if self.space == "device" else v


def make_map(gpu, ops, octaves=None):
    m = gpu.Map()
    lc.apply(m, ops)
    for k, oc in (octaves or {}).items():
        m.SetKeyFrameKeys(k, oc)
    return m


def call_correct(lcl, c, t, kf=None, cur_kf=None, Scw=None):
    return lcl.CorrectLoop(c.kf if kf is None else kf, c.cur_kf if cur_kf is None else cur_kf,
                           c.Scw if Scw is None else Scw, lc.SCALE_FACTORS, t["Tcw"], t["pos"], t["normal"],
                           t["max_dist"], t["min_dist"], t["ref_kf"], t["corrected_ref"], bad=t["bad"])


def check_correct(got, t, want):
    for k in ("Tcw", "pos", "normal", "max_dist", "min_dist"):
        same_bits(t.host(k).reshape(want[k].shape), want[k], k)
    assert np.array_equal(t.host("corrected_ref"), want["corrected_ref"])
    same_bits(got["CorrectedSim3"], want["CorrectedSim3"], "CorrectedSim3")
    same_bits(got["NonCorrectedSim3"], want["NonCorrectedSim3"], "NonCorrectedSim3")
    assert (got["n_corrected"], got["n_ref_missing"]) == (want["n_corrected"], want["n_ref_missing"])


@pytest.mark.parametrize("space", SPACES)
@pytest.mark.parametrize("name", list(CORRECT))
def test_correct_loop_matches_restatement(gpu, want_correct, name, space):
    c, want = CORRECT[name], want_correct[name]
    lcl = gpu.LoopClosing(gpu.ORBmatcher(0.8, False), make_map(gpu, c.ops, c.octaves))
    t = Tables(space, **c.tables())
    check_correct(call_correct(lcl, c, t), t, want)
    assert want["n_corrected"] > 0 and want["n_ref_missing"] > 0
    # the same list in descending id gives the same answer, the Sim3 rows following the list
    t2 = Tables(space, **c.tables())
    rev = np.sort(c.kf)[::-1].copy()
    got = call_correct(lcl, c, t2, kf=rev)
    at = {int(k): j for j, k in enumerate(c.kf)}
    want2 = dict(want, CorrectedSim3=want["CorrectedSim3"][[at[int(k)] for k in rev]],
                 NonCorrectedSim3=want["NonCorrectedSim3"][[at[int(k)] for k in rev]])
    check_correct(got, t2, want2)


@pytest.mark.parametrize("space", SPACES)
def test_correct_loop_follows_the_handles_mutations(gpu, want_correct, space):
    """A second call after Map_EraseKeyFrame of a listed observer and Map_ReplaceMapPoint sees the new relation."""
    c = CORRECT["identity"]
    m = make_map(gpu, c.ops, c.octaves)
    lcl = gpu.LoopClosing(gpu.ORBmatcher(0.8, False), m)
    t = Tables(space, **c.tables())
    check_correct(call_correct(lcl, c, t), t, want_correct["identity"])
    ref = c.refmap()
    shared = sorted(p for p, mp in ref.pts.items() if p >= 4 and len(mp.mObservations) >= 2)
    gone = int(c.kf[1])
    assert gone != c.cur_kf and ref.pts[0].IsInKeyFrame(ref.kfs[gone])
    ops = [("EraseKeyFrame", gone), ("ReplaceMapPoint", shared[0], shared[1])]
    lc.apply(m, ops)
    lc.apply(ref, ops)
    kf = np.array([k for k in c.kf if k != gone], np.int32)
    bad = c.bad.copy()
    bad[shared[0]] = 1
    want = c.restate(ref, kf=kf, bad=bad)
    t2 = Tables(space, **dict(c.tables(), bad=bad))
    check_correct(call_correct(lcl, c, t2, kf=kf), t2, want)
    assert not np.array_equal(want["normal"][0], want_correct["identity"]["normal"][0])   # one observer fewer
    with pytest.raises(OrbGpuError) as e:                                                   # the erased keyframe
        call_correct(lcl, c, t2)
    assert e.value.code == ORB_E_INVALID


def call_gba(lcl, c, t):
    return lcl.ApplyGlobalBA(c.origins, t["TcwGBA"], t["kf_in_gba"], t["Tcw"], t["pos"], t["posGBA"], t["mp_in_gba"],
                             t["ref_kf"], bad=t["bad"], TcwBefGBA=t["TcwBefGBA"], kf_done=t["kf_done"])


def gba_tables(space, c, **over):
    a = dict(TcwGBA=c.TcwGBA, kf_in_gba=c.kf_in_gba, Tcw=c.Tcw, pos=c.pos, posGBA=c.posGBA, mp_in_gba=c.mp_in_gba,
             ref_kf=c.ref_kf, bad=c.bad, TcwBefGBA=np.zeros_like(c.Tcw), kf_done=np.zeros(c.n_kf_rows, np.uint8))
    a.update(over)
    return Tables(space, **a)


@pytest.mark.parametrize("space", SPACES)
@pytest.mark.parametrize("name", list(GBA))
def test_apply_global_ba_matches_restatement(gpu, want_gba, name, space):
    c, want = GBA[name], want_gba[name]
    lcl = gpu.LoopClosing(gpu.ORBmatcher(0.8, False), make_map(gpu, c.ops))
    t = gba_tables(space, c)
    got = call_gba(lcl, c, t)
    for k in ("Tcw", "TcwGBA", "TcwBefGBA", "pos"):
        same_bits(t.host(k).reshape(want[k].shape), want[k], k)
    assert np.array_equal(t.host("kf_done"), want["kf_done"])
    assert got == {k: want[k] for k in ("n_kf_propagated", "n_mp_gba", "n_mp_moved", "depth")}
    # the optional outputs left out
    t2 = gba_tables(space, c, TcwBefGBA=None, kf_done=None)
    assert call_gba(lcl, c, t2) == got
    same_bits(t2.host("Tcw").reshape(want["Tcw"].shape), want["Tcw"], "Tcw")
    same_bits(t2.host("pos").reshape(want["pos"].shape), want["pos"], "pos")


def test_the_gba_cases_reach_what_they_are_named_for(want_gba):
    w = want_gba
    assert w["origin_alone"]["kf_done"].sum() == 1 and w["all_in_ba"]["n_kf_propagated"] == 0
    assert np.array_equal(w["all_in_ba"]["Tcw"][:20], GBA["all_in_ba"].TcwGBA[:20])
    assert (w["mixed_depths"]["depth"], w["chain_70"]["depth"], w["fan_300"]["depth"]) == (5, 70, 1)
    assert w["fan_300"]["n_kf_propagated"] == 300 and w["two_origins"]["kf_done"][:5].all()
    assert not w["unreached"]["kf_done"][5:7].any() and not w["dead_child"]["kf_done"][3:5].any()
    assert np.array_equal(w["unreached"]["Tcw"][5:7], GBA["unreached"].Tcw[5:7])


def expect_invalid(call, t, before):
    with pytest.raises(OrbGpuError) as e:
        call()
    assert e.value.code == ORB_E_INVALID
    for k, v in before.items():
        if v is not None:
            assert np.array_equal(bits(t.host(k)), bits(v)), k


def deferred(matcher, f):
    """f() with the matcher in deferred mode"""
    L = lib()
    assert L.ORBmatcher_set_device_pointers(matcher._h, 1) == 0
    assert L.ORBmatcher_set_deferred(matcher._h, 1) == 0
    try:
        f()
    finally:
        assert L.ORBmatcher_set_deferred(matcher._h, 0) == 0


@pytest.mark.parametrize("space", SPACES)
def test_correct_loop_rejects_bad_arguments_and_leaves_the_tables(gpu, space):
    c = CORRECT["two_listed"]
    m = make_map(gpu, c.ops, c.octaves)
    mt = gpu.ORBmatcher(0.8, False)
    lcl = gpu.LoopClosing(mt, m)
    before = c.tables()
    t = Tables(space, **before)
    free_row = c.n_kf_rows - 1                                   # a row of the table without a keyframe
    bad_s = [c.Scw.copy() for _ in range(4)]
    bad_s[0][7], bad_s[1][7], bad_s[2][4], bad_s[3][0] = 0.0, -1.0, np.inf, np.nan
    calls = [lambda: call_correct(lcl, c, t, kf=np.array([0, 2, free_row], np.int32)),       # not live
             lambda: call_correct(lcl, c, t, kf=np.array([0, 2, 0], np.int32)),              # named twice
             lambda: call_correct(lcl, c, t, kf=np.array([0, 2, c.n_kf_rows], np.int32)),    # id >= n_kf_rows
             lambda: call_correct(lcl, c, t, kf=np.array([0, -1], np.int32), cur_kf=0),
             lambda: call_correct(lcl, c, t, cur_kf=1),                                      # not in the list
             lambda: call_correct(lcl, c, t, kf=np.zeros(0, np.int32))]
    calls += [lambda s=s: call_correct(lcl, c, t, Scw=s) for s in bad_s]
    for k in ("Tcw", "pos", "normal", "max_dist", "min_dist", "ref_kf", "corrected_ref"):   # a missing array
        calls.append(lambda k=k: call_correct(lcl, c, dict(t.a, **{k: None})))
    for call in calls:
        expect_invalid(call, t, before)
    if space == "device":                                        # a deferred matcher (device pointers only)
        deferred(mt, lambda: expect_invalid(lambda: call_correct(lcl, c, t), t, before))
    m.SetNeighbours(0, [], 1, [1])                               # a cycle in the children relation
    m.SetNeighbours(1, [], 0, [0])
    expect_invalid(lambda: call_correct(lcl, c, t), t, before)
    m.SetNeighbours(1, [], 0, [])
    call_correct(lcl, c, t)                                      # and the well-formed call still runs
    assert not np.array_equal(t.host("pos"), before["pos"])


@pytest.mark.parametrize("space", SPACES)
def test_apply_global_ba_rejects_bad_arguments_and_leaves_the_tables(gpu, space):
    c = GBA["mixed_depths"]
    m = make_map(gpu, c.ops)
    mt = gpu.ORBmatcher(0.8, False)
    lcl = gpu.LoopClosing(mt, m)
    t = gba_tables(space, c)
    before = {k: (None if v is None else t.host(k).copy()) for k, v in t.a.items()}

    def call(origins=None, **over):
        a = dict(t.a, **over)
        return lcl.ApplyGlobalBA(c.origins if origins is None else origins, a["TcwGBA"], a["kf_in_gba"], a["Tcw"],
                                 a["pos"], a["posGBA"], a["mp_in_gba"], a["ref_kf"], bad=a["bad"],
                                 TcwBefGBA=a["TcwBefGBA"], kf_done=a["kf_done"])

    calls = [lambda: call(origins=[2]),                          # an origin that is not in the BA
             lambda: call(origins=[0, c.n_kf_rows]),             # id >= n_kf_rows
             lambda: call(origins=[-1])]
    for k in ("TcwGBA", "kf_in_gba", "Tcw", "pos", "posGBA", "mp_in_gba", "ref_kf"):
        calls.append(lambda k=k: call(**{k: None}))
    for f in calls:
        expect_invalid(f, t, before)
    if space == "device":
        deferred(mt, lambda: expect_invalid(call, t, before))
    m.SetNeighbours(2, [], 1, [1])                               # 1 -> 2 -> 1
    expect_invalid(call, t, before)
    m.SetNeighbours(2, [], 1, [])
    assert call()["depth"] == 5


def test_a_keyframe_id_beyond_the_pose_table_is_rejected(gpu):
    c = CORRECT["one_listed"]
    lcl = gpu.LoopClosing(gpu.ORBmatcher(0.8, False), make_map(gpu, c.ops, c.octaves))
    before = c.tables()
    before["Tcw"] = before["Tcw"][:2].copy()                     # the handle knows keyframe 2
    t = Tables("host", **before)
    expect_invalid(lambda: call_correct(lcl, c, t), t, before)
