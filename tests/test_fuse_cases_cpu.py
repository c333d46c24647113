"""The inputs of the SearchInNeighbors tests and the entry's argument checks.  No GPU is needed.

The first half runs the reference (tests/fuse_ref.py) alone over the main cases of tests/fuse_cases.py and
requires that they reach what the GPU parity test relies on them for: every kind of mutation, both Replace
directions, several points on one keypoint within a pass, backward-pass fusions, a point whose reference
keyframe is missing, and an op log that the frozen-descriptor variant (stale=True) gets wrong.  The second
half calls LocalMapping_SearchInNeighbors without a device: a malformed call answers ORB_E_INVALID before
the handles are looked at, a well-formed one on NULL handles answers ORB_E_NODEVICE."""
import ctypes as C
import re

import numpy as np
import pytest

import fuse_cases as fc
from c_orb_slam_amd import _lib
from c_orb_slam_amd._lib import ORB_E_INVALID, ORB_E_NODEVICE, device_available, lib, orb_frame, orb_searchneigh, ptr
from fuse_ref import SearchInNeighborsRef


@pytest.fixture(scope="module")
def runs():
    out = {}
    for name in fc.MAIN + fc.EDGE:
        c = fc.case(name)
        out[name] = (c, SearchInNeighborsRef(c.refmap(), *c.args(c.table)).run())
    return out


@pytest.mark.parametrize("name", fc.MAIN)
def test_main_cases_reach_every_outcome(runs, name):
    c, r = runs[name]
    res = r.result()
    kind = res["ops"][:, 1]
    nt = len(c.target_ids)
    seen = dict(add=int((kind == 1).sum()), replaced_examined=r.replaced_examined, replaced_held=r.replaced_held,
                noop=int((kind == 3).sum()), same_keypoint=r.same_keypoint, backward=int(res["nfused"][nt]),
                ref_missing=res["n_ref_missing"])
    print(name, seen, "nfused", res["nfused"].tolist(), "points", c.n_pts)
    assert seen["add"] >= 5 and seen["replaced_examined"] >= 3 and seen["replaced_held"] >= 3, seen
    assert seen["noop"] >= 1 and seen["same_keypoint"] >= 2 and seen["backward"] >= 3 and seen["ref_missing"] >= 1, seen
    assert r.replaced_examined + r.replaced_held == int((kind == 2).sum())
    assert int(res["nfused"].sum()) == len(kind)
    stale = SearchInNeighborsRef(c.refmap(), *c.args(c.table), stale=True).run().result()
    assert not np.array_equal(stale["ops"], res["ops"]), "frozen descriptors give the same op log"


def test_cases_stay_small(runs):
    for name, (c, r) in runs.items():
        assert c.n_pts <= 2000 and len(c.ghost_ids) <= 8 and 4 <= len(c.real_ids) <= 5, name
        # the extractor is asked for 600 features; its octree distribution may return a few more
        assert all(F.N <= 660 for F in c.frames.values()), (name, [F.N for F in c.frames.values()])


def test_edge_cases_are_what_they_say(runs):
    c, r = runs["no_targets"]
    assert c.target_ids == [] and r.result()["nfused"].tolist() == [0] and len(r.result()["ops"]) == 0
    assert len(r.result()["updated"]) > 100            # the final update still runs over the current row
    c, r = runs["empty_cur"]
    nf = r.result()["nfused"]
    assert (nf[:-1] == 0).all() and nf[-1] >= 3 and c.cur.N > 0
    c, r = runs["twice"]
    assert len(set(c.target_ids)) < len(c.target_ids)
    assert r.result()["nfused"][len(c.target_ids) - 1] >= 1, "the second pass into the same keyframe fuses nothing"
    c, r = runs["one_target"]
    assert len(c.target_ids) == 1


def test_the_final_update_follows_the_float64_formulas(runs):
    for name, (c, r) in runs.items():
        assert len(r.final_rows) > 0 or name == "empty_cur"
        assert r.float64_deviation(r.t["normal"], r.t["max_dist"], r.t["min_dist"]) <= 1.0, name


def test_replaced_points_leave_every_row(runs):
    for name, (c, r) in runs.items():
        gone = set(int(a) for a in r.result()["ops"][r.result()["ops"][:, 1] == 2][:, 2])
        for kf in r.ref.kfs.values():
            ids = [m.mnId for m in kf.mvpMapPoints if m is not None]
            assert len(ids) == len(set(ids)) and not gone & set(ids), name
        assert all(r.t["bad"][a] for a in gone)


# ---------------------------------------------------------------- the C ABI without a device
class Call:
    """A well-formed orb_searchneigh over the "one_target" case, with everything it points to kept alive."""

    def __init__(self):
        c = fc.case("one_target")
        self.c = c
        self.t = c.table_copy()
        self.Ow = np.ascontiguousarray(c.Ow, np.float32)
        self.dptr = (C.c_void_p * c.n_kf_rows)()
        self.rows = {k: np.ascontiguousarray(d) for k, d in c.kf_desc.items()}
        for k, d in self.rows.items():
            self.dptr[k] = d.ctypes.data if d.size else None
        self.tid = np.array(c.target_ids, np.int32)
        self.fr = (orb_frame * len(self.tid))(*[F.cstruct() for F in c.targets])
        self.fc = c.cur.cstruct()
        self.sf = np.ascontiguousarray(c.scale, np.float32)
        self.nfused, self.ops, self.upd = np.zeros(2, np.int32), np.zeros((64, 6), np.int32), np.zeros(64, np.int32)
        S = orb_searchneigh()
        S.cur_kf, S.cur, S.ntargets, S.target_id, S.target = c.cur_kf, C.pointer(self.fc), 1, ptr(self.tid), self.fr
        S.th, S.logScaleFactor, S.n_kf_rows = 3.0, float(fc.LOG_SF), c.n_kf_rows
        S.kf_desc, S.Ow, S.nlevels, S.scale_factors = C.cast(self.dptr, C.c_void_p), ptr(self.Ow), len(self.sf), ptr(self.sf)
        S.n = c.n_pts
        for k in ("pos", "desc", "normal", "max_dist", "min_dist", "bad", "ref_kf"):
            setattr(S, k, ptr(self.t[k]))
        S.apply, S.cap_ops, S.cap_updated = 1, 64, 64
        S.nfused, S.ops, S.updated = ptr(self.nfused), ptr(self.ops), ptr(self.upd)
        self.S = S

    def run(self):
        return lib().LocalMapping_SearchInNeighbors(None, None, C.byref(self.S))


def test_malformed_calls_answer_invalid_before_the_handles():
    assert lib().LocalMapping_SearchInNeighbors(None, None, None) == ORB_E_INVALID
    null = C.c_void_p(None)
    for field in ("cur", "target_id", "target", "kf_desc", "Ow", "scale_factors", "pos", "desc", "normal", "max_dist",
                  "min_dist", "bad", "ref_kf", "nfused", "ops", "updated"):
        k = Call()
        setattr(k.S, field, C.POINTER(orb_frame)() if field in ("cur", "target") else null)
        assert k.run() == ORB_E_INVALID, field
    for field, value in (("ntargets", -1), ("n_kf_rows", 0), ("nlevels", 0), ("n", -1), ("cap_ops", -1),
                         ("cap_updated", -1), ("cur_kf", -1), ("cur_kf", 18), ("th", float("nan")),
                         ("logScaleFactor", 0.0)):
        k = Call()
        setattr(k.S, field, value)
        assert k.run() == ORB_E_INVALID, (field, value)
    k = Call()
    k.tid[0] = k.c.cur_kf                     # the current keyframe among the targets
    assert k.run() == ORB_E_INVALID
    k = Call()
    k.tid[0] = k.c.n_kf_rows                  # an id beyond the keyframe tables
    assert k.run() == ORB_E_INVALID
    k = Call()
    k.fr[0].N = 5000                          # beyond the keypoint limit of a row
    assert k.run() == ORB_E_INVALID
    k = Call()
    keys = k.c.targets[0].keysUn.copy()
    keys["octave"][3] = 8                     # an octave outside [0, nlevels)
    k.fr[0].keysUn = keys.ctypes.data
    assert k.run() == ORB_E_INVALID
    k = Call()
    k.fc.Tcw = None
    assert k.run() == ORB_E_INVALID
    assert lib().LocalMapping_SearchInNeighbors_last_timings(None, None) == ORB_E_INVALID


def test_a_well_formed_call_on_null_handles():
    k = Call()
    before = {name: a.copy() for name, a in k.t.items()}
    assert k.run() == (ORB_E_INVALID if device_available() else ORB_E_NODEVICE)
    assert all(np.array_equal(before[name], k.t[name]) for name in before)
    ms = np.zeros(5, np.float32)
    assert lib().LocalMapping_SearchInNeighbors_last_timings(None, ptr(ms)) == (
        ORB_E_INVALID if device_available() else ORB_E_NODEVICE)


def test_header_declares_and_binding_binds_the_entry():
    names = _lib.header_functions()
    src = (_lib.PKG / "_lib.py").read_text()
    for f in ("LocalMapping_SearchInNeighbors", "LocalMapping_SearchInNeighbors_last_timings"):
        assert f in names
        assert re.search(rf"L\.{f}\.argtypes", src)
    header = _lib.HEADER.read_text()
    assert re.search(r"#define\s+ORBGPU_ABI_VERSION\s+2\b", header)
    assert lib().orbgpu_abi_version() == 2
    import c_orb_slam_amd
    assert hasattr(c_orb_slam_amd.Map, "SearchInNeighbors")
