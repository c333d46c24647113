"""The inputs of the LoopClosing_SearchAndFuse tests and the entry's argument checks.  No GPU is needed.

The first half runs the reference (tests/loopfuse_ref.py) alone over the main cases of tests/loopfuse_cases.py
and requires that they reach what the GPU parity test relies on them for: every kind of mutation in the passes
and in step 0, points that choose a keypoint another point of the pass took, Replaces of an already-dead
point, loop points replaced by loop points, survivors whose descriptor moves, and an op log that the
plan-every-keyframe-first adapter gets wrong.  These are conditions on the inputs, not measurements.  The
second half calls LoopClosing_SearchAndFuse without a device: a malformed call answers ORB_E_INVALID before
the handles are looked at, a well-formed one on NULL handles answers ORB_E_NODEVICE."""
import ctypes as C
import re

import numpy as np
import pytest

import loopfuse_cases as lc
from c_orb_slam_amd import _lib
from c_orb_slam_amd._lib import (ORB_E_INVALID, ORB_E_NODEVICE, device_available, lib, orb_frame, orb_loopfuse,
                                 ptr)
from loopfuse_ref import SearchAndFuseRef, cvScw_of


def run_ref(c, **kw):
    return SearchAndFuseRef(c.refmap(), **c.kwargs(c.table), **kw).run()


@pytest.fixture(scope="module")
def runs():
    return {name: (lc.case(name), run_ref(lc.case(name))) for name in lc.MAIN + lc.EDGE}


@pytest.mark.parametrize("name", lc.MAIN)
def test_main_cases_reach_every_outcome(runs, name):
    c, r = runs[name]
    res = r.result()
    ops = res["ops"]
    step0, passes = ops[ops[:, 0] < 0], ops[ops[:, 0] >= 0]
    seen = dict(adds=int((passes[:, 1] == 1).sum()), replaces=int((passes[:, 1] == 2).sum()),
                kind3=int((passes[:, 1] == 3).sum()), same_keypoint=r.same_keypoint, dead_replaced=r.dead_replaced,
                loop_by_loop=r.loop_by_loop, desc_changed=len(r.desc_changed),
                step0_replaces=int((step0[:, 1] == 2).sum()), step0_adds=int((step0[:, 1] == 1).sum()),
                step0_same=r.step0_same)
    print(name, seen, "nfused", res["nfused"].tolist(), "kf", c.kf, "points", c.n_pts)
    assert seen["adds"] >= 50 and seen["replaces"] >= 50 and seen["kind3"] >= 1, seen
    assert seen["same_keypoint"] >= 5 and seen["dead_replaced"] >= 3 and seen["loop_by_loop"] >= 5, seen
    assert seen["desc_changed"] >= 20, seen
    assert seen["step0_replaces"] >= 10 and seen["step0_adds"] >= 10 and seen["step0_same"] >= 5, seen
    assert int(res["nfused"].sum()) == len(passes)
    assert len(step0) == r.n_step0_ops and (ops[:r.n_step0_ops, 0] == -1).all()
    wrong = run_ref(c, plan_first=True).result()
    assert not np.array_equal(wrong["ops"], ops), "planning every keyframe first gives the same op log"
    assert c.kf != sorted(c.kf), "the caller's order is the pass order"


def test_cases_stay_small(runs):
    for name, (c, r) in runs.items():
        assert c.n_pts <= 2000 and len(c.base.real_ids) <= 5 and len(c.kf) <= 4, name
        assert all(F.N <= 660 for F in c.frames), name
        assert len(c.loop_pts) <= 660, name


def test_edge_cases_are_what_they_say(runs):
    c, r = runs["no_keyframes"]
    assert c.kf == [] and c.matched is None and len(r.result()["ops"]) == 0 and len(r.result()["nfused"]) == 0
    c, r = runs["empty_loop"]
    assert len(c.loop_pts) == 0 and len(c.kf) == 4 and r.result()["nfused"].tolist() == [0] * 4
    c, r = runs["no_matched"]
    assert c.matched is None and (r.result()["ops"][:, 0] >= 0).all() and r.result()["nfused"].sum() > 50
    c, r = runs["one_keyframe"]
    assert len(c.kf) == 1 and c.cur_kf == c.kf[0] and r.result()["nfused"][0] > 50
    c, r = runs["matched_held_twice"]
    res, tw = r.result(), c.twice
    assert res["n_matched_skipped"] == 1
    first = [tuple(int(v) for v in o) for o in res["ops"][res["ops"][:, 0] < 0]]
    assert first == [(-1, 2, tw["replaced"], tw["L"], c.cur_kf, tw["held"])]
    row0 = c.refmap().kfs[c.cur_kf].mvpMapPoints            # the row before the call
    assert row0[tw["at"]].mnId == tw["L"] and row0[tw["held"]].mnId == tw["replaced"] and row0[tw["empty"]] is None
    assert r.t["bad"][tw["replaced"]] and not c.table["bad"][tw["replaced"]]
    assert all(runs[n][1].result()["n_matched_skipped"] == 0 for n in lc.MAIN)


def test_replaced_points_leave_every_row(runs):
    for name, (c, r) in runs.items():
        ops = r.result()["ops"]
        gone = set(int(a) for a in ops[ops[:, 1] == 2][:, 2])
        for kf in r.ref.kfs.values():
            ids = [m.mnId for m in kf.mvpMapPoints if m is not None]
            assert len(ids) == len(set(ids)) and not gone & set(ids), name
        assert all(r.t["bad"][a] for a in gone)
        for k in ("pos", "normal", "max_dist", "min_dist"):
            assert np.array_equal(r.t[k], c.table[k])


def test_the_sim3_of_a_case_reproduces_its_pose():
    """Scw = (q(R), s t, s): the decomposition gives back Rcw = R and tcw = t up to float rounding."""
    c = lc.case("stereo")
    for kid, F in zip(c.kf, c.frames):
        S = cvScw_of(c.scw_of[kid]).astype(np.float64)
        s = np.sqrt((S[0, :3] ** 2).sum())
        assert abs(s - c.scw_of[kid][7]) < 1e-6
        assert np.abs(S[:3, :3] / s - F.Tcw[:3, :3]).max() < 1e-6 and np.abs(S[:3, 3] / s - F.Tcw[:3, 3]).max() < 1e-6
    assert len(set(c.scw_of[k][7] for k in c.kf)) == len(c.kf)


# ---------------------------------------------------------------- the C ABI without a device
class Call:
    """A well-formed orb_loopfuse over the "one_keyframe" case, with everything it points to kept alive."""

    def __init__(self):
        c = lc.case("one_keyframe")
        self.c = c
        self.t = c.table_copy()
        self.dptr = (C.c_void_p * c.n_kf_rows)()
        self.rows = {k: np.ascontiguousarray(d) for k, d in c.kf_desc.items()}
        for k, d in self.rows.items():
            self.dptr[k] = d.ctypes.data if d.size else None
        self.kf = np.array(c.kf, np.int32)
        self.fr = (orb_frame * len(self.kf))(*[F.cstruct() for F in c.frames])
        self.Scw = np.ascontiguousarray(c.Scw)
        self.loop = np.array(c.loop_pts, np.int32)           # copies: the calls below change them
        self.matched = np.array(c.matched, np.int32)
        self.nfused, self.ops, self.upd = np.zeros(1, np.int32), np.zeros((64, 6), np.int32), np.zeros(64, np.int32)
        S = orb_loopfuse()
        S.nkf, S.kf, S.frame, S.Scw = 1, ptr(self.kf), self.fr, ptr(self.Scw)
        S.nloop, S.loop_pts = len(self.loop), ptr(self.loop)
        S.cur_kf, S.nmatched, S.matched = c.cur_kf, len(self.matched), ptr(self.matched)
        S.th, S.logScaleFactor, S.n_kf_rows = 4.0, float(lc.LOG_SF), c.n_kf_rows
        S.kf_desc, S.n = C.cast(self.dptr, C.c_void_p), c.n_pts
        for k in ("pos", "normal", "max_dist", "min_dist", "desc", "bad"):
            setattr(S, k, ptr(self.t[k]))
        S.apply, S.cap_ops, S.cap_updated = 1, 64, 64
        S.nfused, S.ops, S.updated = ptr(self.nfused), ptr(self.ops), ptr(self.upd)
        self.S = S

    def run(self):
        return lib().LoopClosing_SearchAndFuse(None, None, C.byref(self.S))


def test_malformed_calls_answer_invalid_before_the_handles():
    assert lib().LoopClosing_SearchAndFuse(None, None, None) == ORB_E_INVALID
    null = C.c_void_p(None)
    for field in ("kf", "frame", "Scw", "loop_pts", "kf_desc", "pos", "normal", "max_dist", "min_dist", "desc", "bad",
                  "nfused", "ops", "updated"):
        k = Call()
        setattr(k.S, field, C.POINTER(orb_frame)() if field == "frame" else null)
        assert k.run() == ORB_E_INVALID, field
    for field, value in (("nkf", -1), ("nloop", -1), ("nmatched", -1), ("n_kf_rows", 0), ("n", -1), ("cap_ops", -1),
                         ("cap_updated", -1), ("cur_kf", -1), ("cur_kf", 18), ("th", float("nan")),
                         ("logScaleFactor", 0.0)):
        k = Call()
        setattr(k.S, field, value)
        assert k.run() == ORB_E_INVALID, (field, value)
    k = Call()
    k.kf[0] = k.c.n_kf_rows                    # a listed id beyond the keyframe tables
    assert k.run() == ORB_E_INVALID
    k = Call()                                 # a keyframe named twice
    k.kf = np.array([k.c.kf[0]] * 2, np.int32)
    k.fr = (orb_frame * 2)(*[k.c.frames[0].cstruct()] * 2)
    k.Scw = np.ascontiguousarray(np.tile(k.c.Scw, (2, 1)))
    k.nfused = np.zeros(2, np.int32)
    k.S.nkf, k.S.kf, k.S.frame, k.S.Scw, k.S.nfused = 2, ptr(k.kf), k.fr, ptr(k.Scw), ptr(k.nfused)
    assert k.run() == ORB_E_INVALID
    k = Call()
    held = np.flatnonzero(k.loop >= 0)
    k.loop[held[1]] = k.loop[held[0]]          # loop_pts holding an id twice
    assert k.run() == ORB_E_INVALID
    k = Call()
    k.loop[held[0]] = k.c.n_pts                # a loop id beyond the table
    assert k.run() == ORB_E_INVALID
    k = Call()
    k.fr[0].N = 5000                           # beyond the keypoint limit of a row
    assert k.run() == ORB_E_INVALID
    k = Call()
    keys = k.c.frames[0].keysUn.copy()
    keys["octave"][3] = 8                      # an octave outside [0, nlevels)
    k.fr[0].keysUn = keys.ctypes.data
    assert k.run() == ORB_E_INVALID
    for j, value in ((0, float("nan")), (5, float("inf")), (7, 0.0), (7, -1.0)):   # a non-finite Scw, s <= 0
        k = Call()
        k.Scw[0, j] = value
        assert k.run() == ORB_E_INVALID, (j, value)
    k = Call()
    at = int(np.flatnonzero(k.matched >= 0)[0])
    k.matched[at] = k.c.n_pts                  # a matched id beyond the table
    assert k.run() == ORB_E_INVALID
    k = Call()
    k.t["bad"][k.matched[at]] = 1              # a matched id that is bad when the call starts
    assert k.run() == ORB_E_INVALID
    assert lib().LoopClosing_SearchAndFuse_last_timings(None, None) == ORB_E_INVALID


def test_a_well_formed_call_on_null_handles():
    k = Call()
    before = {name: a.copy() for name, a in k.t.items()}
    assert k.run() == (ORB_E_INVALID if device_available() else ORB_E_NODEVICE)
    assert all(np.array_equal(before[name], k.t[name]) for name in before)
    k = Call()
    k.fr[0].Tcw = None                         # Tcw is not read
    k.S.matched = C.c_void_p(None)             # no step 0: cur_kf is not read either
    k.S.cur_kf = -1
    assert k.run() == (ORB_E_INVALID if device_available() else ORB_E_NODEVICE)
    ms = np.zeros(4, np.float32)
    assert lib().LoopClosing_SearchAndFuse_last_timings(None, ptr(ms)) == (
        ORB_E_INVALID if device_available() else ORB_E_NODEVICE)


def test_header_declares_and_binding_binds_the_entry():
    names = _lib.header_functions()
    src = (_lib.PKG / "_lib.py").read_text()
    for f in ("LoopClosing_SearchAndFuse", "LoopClosing_SearchAndFuse_last_timings"):
        assert f in names
        assert re.search(rf"L\.{f}\.argtypes", src)
    header = _lib.HEADER.read_text()
    assert re.search(r"#define\s+ORBGPU_ABI_VERSION\s+2\b", header)
    assert lib().orbgpu_abi_version() == 2
    assert "typedef struct orb_loopfuse" in header and hasattr(_lib, "orb_loopfuse")
    from c_orb_slam_amd.loop_closing import LoopClosing
    assert hasattr(LoopClosing, "SearchAndFuse")
