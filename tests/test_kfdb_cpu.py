"""CPU: the KeyFrameDatabase entry points' argument validation (before the device), the
restatement tests/kfdb_ref.py pinned against the vocabulary oracle's score and against hand-built
boundary cases, the closed-form order of lKFsSharingWords, and the non-vacuity of the cases the
GPU tests compare (conditions on the inputs, asserted on the restatement alone).

Reference: src/KeyFrameDatabase.cc (add 39-45, erase 47-67, clear 69-73, DetectLoopCandidates
76-197, DetectRelocalizationCandidates 199-309)."""
import ctypes as C

import numpy as np
import pytest

import kfdb_cases as kc
import kfdb_ref as kr
import oracle_lib
import vocab_cases as vc
import c_orb_slam_amd as orb
from c_orb_slam_amd._lib import (ORB_E_INVALID, ORB_E_NODEVICE, header_functions, lib, orb_kfdb_query,
                                 orb_kfdb_result, ptr)

NAMES = ["KeyFrameDatabase_create", "KeyFrameDatabase_destroy", "KeyFrameDatabase_add", "KeyFrameDatabase_add_batch",
         "KeyFrameDatabase_erase", "KeyFrameDatabase_clear", "KeyFrameDatabase_size",
         "KeyFrameDatabase_set_covisibles", "KeyFrameDatabase_DetectLoopCandidates",
         "KeyFrameDatabase_DetectRelocalizationCandidates", "KeyFrameDatabase_DetectRelocalizationCandidates_batch",
         "KeyFrameDatabase_enable_timing", "KeyFrameDatabase_last_timings", "orbgpu_unit_set_kfdb_initial_capacity"]


@pytest.fixture(scope="module")
def results():
    """The restatement's stages for every query step of every GPU case, computed once."""
    return {c["name"]: (c, kr.run_steps(c["steps"], kc.n_words(c["vocab"]))) for c in kc.gpu_cases()}


def _flat(outs):
    for o in outs:
        yield from (o if isinstance(o, list) else [o])


def _queries(case):
    """(kind, bow, connected ids, minScore) of every query, batches flattened, in step order."""
    for s in case["steps"]:
        if s[0] == "loop":
            yield "loop", s[1], s[2], s[3]
        elif s[0] == "reloc":
            yield "reloc", s[1], [], None
        elif s[0] == "reloc_batch":
            for b in s[1]:
                yield "reloc", b, [], None


def test_symbols_exported_and_declared():
    L = lib()
    hdr = header_functions()
    for n in NAMES:
        assert n in hdr, n
        assert getattr(L, n).argtypes is not None, n
    assert orb.KeyFrameDatabase is not None and "KeyFrameDatabase" in dir(orb)


def test_argument_validation_comes_before_the_device(tmp_path):
    L = lib()
    p = tmp_path / "tiny.txt"
    vc.tiny_vocab(p)
    voc = orb.ORBVocabulary()
    assert voc.loadFromTextFile(p)
    nodev = not orb.device_available()
    valid_null = ORB_E_NODEVICE if nodev else ORB_E_INVALID   # an otherwise valid call on a NULL handle
    h = C.c_void_p()
    assert L.KeyFrameDatabase_create(None, C.byref(h)) == ORB_E_INVALID
    assert L.KeyFrameDatabase_create(voc._h, None) == ORB_E_INVALID
    if nodev:
        assert L.KeyFrameDatabase_create(voc._h, C.byref(h)) == ORB_E_NODEVICE and not h
        with pytest.raises(orb.OrbGpuError) as ei:
            orb.KeyFrameDatabase(voc)
        assert ei.value.code == ORB_E_NODEVICE
    assert L.KeyFrameDatabase_destroy(None) == ORB_E_INVALID
    w, v = np.array([0, 1, 3], np.uint32), np.array([0.5, 0.25, 0.25])
    # add
    assert L.KeyFrameDatabase_add(None, 1, None, ptr(v), 3) == ORB_E_INVALID
    assert L.KeyFrameDatabase_add(None, 1, ptr(w), None, 3) == ORB_E_INVALID
    assert L.KeyFrameDatabase_add(None, 1, ptr(w), ptr(v), -1) == ORB_E_INVALID
    assert L.KeyFrameDatabase_add(None, -1, ptr(w), ptr(v), 3) == ORB_E_INVALID
    big_w, big_v = np.arange(4097, dtype=np.uint32), np.full(4097, 1 / 4097)
    assert L.KeyFrameDatabase_add(None, 1, ptr(big_w), ptr(big_v), 4097) == ORB_E_INVALID
    for bad in ([0, 3, 1], [0, 1, 1]):                        # not strictly ascending
        bw = np.array(bad, np.uint32)
        assert L.KeyFrameDatabase_add(None, 1, ptr(bw), ptr(v), 3) == ORB_E_INVALID
    assert L.KeyFrameDatabase_add(None, 1, ptr(w), ptr(v), 3) == valid_null
    assert L.KeyFrameDatabase_add(None, 1, None, None, 0) == valid_null
    # add_batch
    ids = np.array([4, 5], np.int32)
    ww, vv = np.array([0, 1, 0, 3], np.uint32), np.full(4, 0.5)
    st = np.array([0, 2, 4], np.int32)
    assert L.KeyFrameDatabase_add_batch(None, -1, ptr(ids), ptr(st), ptr(ww), ptr(vv)) == ORB_E_INVALID
    assert L.KeyFrameDatabase_add_batch(None, 2, None, ptr(st), ptr(ww), ptr(vv)) == ORB_E_INVALID
    assert L.KeyFrameDatabase_add_batch(None, 2, ptr(ids), None, ptr(ww), ptr(vv)) == ORB_E_INVALID
    assert L.KeyFrameDatabase_add_batch(None, 2, ptr(ids), ptr(st), None, ptr(vv)) == ORB_E_INVALID
    dec = np.array([0, 3, 2], np.int32)                        # starts decrease
    assert L.KeyFrameDatabase_add_batch(None, 2, ptr(ids), ptr(dec), ptr(ww), ptr(vv)) == ORB_E_INVALID
    off = np.array([1, 2, 4], np.int32)                        # start[0] != 0
    assert L.KeyFrameDatabase_add_batch(None, 2, ptr(ids), ptr(off), ptr(ww), ptr(vv)) == ORB_E_INVALID
    assert L.KeyFrameDatabase_add_batch(None, 2, ptr(ids), ptr(st), ptr(ww), ptr(vv)) == valid_null
    # set_covisibles
    c11 = np.arange(11, dtype=np.int32)
    assert L.KeyFrameDatabase_set_covisibles(None, 1, 11, ptr(c11)) == ORB_E_INVALID
    assert L.KeyFrameDatabase_set_covisibles(None, 1, -1, ptr(c11)) == ORB_E_INVALID
    assert L.KeyFrameDatabase_set_covisibles(None, 1, 3, None) == ORB_E_INVALID
    assert L.KeyFrameDatabase_set_covisibles(None, 1, 10, ptr(c11)) == valid_null
    # queries
    cand = np.zeros(8, np.int32)

    def Q(nq=3, word=w, value=v, nex=0, ex=None):
        return orb_kfdb_query(nq, ptr(word) if word is not None else None, ptr(value) if value is not None else None,
                              nex, ptr(ex) if ex is not None else None, 0.0)

    def R(cap=8, c=cand, cap_scored=0):
        return orb_kfdb_result(cap, ptr(c) if c is not None else None, 0, cap_scored, None, None, None, None, 0, 0, 0,
                               0, 0.0)

    for fn in (L.KeyFrameDatabase_DetectLoopCandidates, L.KeyFrameDatabase_DetectRelocalizationCandidates):
        r = R()
        assert fn(None, None, C.byref(r)) == ORB_E_INVALID
        assert fn(None, C.byref(Q()), None) == ORB_E_INVALID
        assert fn(None, C.byref(Q(nq=-1)), C.byref(r)) == ORB_E_INVALID
        assert fn(None, C.byref(Q(nq=4097, word=big_w, value=big_v)), C.byref(r)) == ORB_E_INVALID
        assert fn(None, C.byref(Q(word=None)), C.byref(r)) == ORB_E_INVALID
        assert fn(None, C.byref(Q(value=None)), C.byref(r)) == ORB_E_INVALID
        unsorted = np.array([2, 1, 3], np.uint32)
        assert fn(None, C.byref(Q(word=unsorted)), C.byref(r)) == ORB_E_INVALID
        assert fn(None, C.byref(Q()), C.byref(R(cap=-1))) == ORB_E_INVALID
        assert fn(None, C.byref(Q()), C.byref(R(cap=4, c=None))) == ORB_E_INVALID
        assert fn(None, C.byref(Q()), C.byref(R(cap_scored=-1))) == ORB_E_INVALID
        assert fn(None, C.byref(Q()), C.byref(r)) == valid_null
        assert fn(None, C.byref(Q(nq=0, word=None, value=None)), C.byref(r)) == valid_null
    r = R()
    assert L.KeyFrameDatabase_DetectLoopCandidates(None, C.byref(Q(nex=-1)), C.byref(r)) == ORB_E_INVALID
    assert L.KeyFrameDatabase_DetectLoopCandidates(None, C.byref(Q(nex=2)), C.byref(r)) == ORB_E_INVALID
    qa = (orb_kfdb_query * 2)(Q(), Q(nq=-1))
    ra = (orb_kfdb_result * 2)(R(), R())
    fb = L.KeyFrameDatabase_DetectRelocalizationCandidates_batch
    assert fb(None, -1, qa, ra) == ORB_E_INVALID
    assert fb(None, 2, None, ra) == ORB_E_INVALID
    assert fb(None, 2, qa, None) == ORB_E_INVALID
    assert fb(None, 2, qa, ra) == ORB_E_INVALID                # the second query is malformed
    assert fb(None, 1, qa, ra) == valid_null
    assert L.KeyFrameDatabase_last_timings(None, None) == ORB_E_INVALID
    for fn, args in ((L.KeyFrameDatabase_erase, (3,)), (L.KeyFrameDatabase_clear, ()),
                     (L.KeyFrameDatabase_size, (None, None)), (L.KeyFrameDatabase_enable_timing, (1,))):
        assert fn(None, *args) == valid_null
    assert L.orbgpu_unit_set_kfdb_initial_capacity(-1, 4) == 1
    assert L.orbgpu_unit_set_kfdb_initial_capacity(4, -1) == 1
    assert L.orbgpu_unit_set_kfdb_initial_capacity(0, 0) == 0


def test_restatement_score_equals_the_oracle(tmp_path):
    """L1Scoring::score of the restatement against oracle/dbow2.c on 50 seeded pairs, bit for bit."""
    p = tmp_path / "tiny.txt"
    vc.tiny_vocab(p)
    o = oracle_lib.OracleVocabulary(p)
    rng = np.random.default_rng(5)
    nonzero = 0
    for i in range(50):
        n1, n2 = int(rng.integers(0, 200)), int(rng.integers(1, 200))
        a = kc.make_bow(rng, rng.choice(400, size=n1, replace=False))
        b = kc.make_bow(rng, rng.choice(400, size=n2, replace=False))
        s = kr.l1_score((a[0].tolist(), a[1].tolist()), (b[0].tolist(), b[1].tolist()))
        assert np.float64(s).view(np.uint64) == np.float64(o.score(a[0], a[1], b[0], b[1])).view(np.uint64), i
        nonzero += s != 0
    assert nonzero >= 40


def test_sharing_order_is_the_closed_form(results):
    """lKFsSharingWords of the restatement (a walk of the inverted file) equals the sharing
    keyframes sorted by (index in the query of the first shared word, add sequence number), on every
    GPU case, the ones with erase and re-add included."""
    checked = 0
    for case, outs in results.values():
        live, seq = {}, 0                     # id -> (sequence number, set of words)
        it = _flat(outs)
        for s in case["steps"]:
            if s[0] == "add":
                live[s[1]] = (seq, set(s[2][0].tolist()))
                seq += 1
            elif s[0] == "add_batch":
                for i, b in zip(s[1], s[2]):
                    live[i] = (seq, set(b[0].tolist()))
                    seq += 1
            elif s[0] == "erase":
                live.pop(s[1], None)
            elif s[0] == "clear":
                live.clear()
            elif s[0] in ("loop", "reloc", "reloc_batch"):
                for b in (s[1] if s[0] == "reloc_batch" else [s[1]]):
                    st = next(it)
                    ex = set(s[2]) if s[0] == "loop" else set()
                    qw = b[0].tolist()
                    keys = []
                    for kid, (sq, ws) in live.items():
                        first = next((i for i, w in enumerate(qw) if w in ws), None)
                        if first is not None and kid not in ex:
                            keys.append((first, sq, kid))
                    assert st.sharing_ids == [k[2] for k in sorted(keys)], case["name"]
                    checked += 1
    assert checked >= 40


def test_cases_are_not_vacuous(results):
    normal = [(c, o) for c, o in results.values() if c["kind"] == "normal"]
    assert len(normal) >= 10
    sts, loops = [], []
    for case, outs in normal:
        qs = list(_queries(case))
        flat = list(_flat(outs))
        assert len(qs) == len(flat)
        for (kind, bow, con, ms), st in zip(qs, flat):
            assert len(st.cand) >= 1, (case["name"], kind)
            sts.append(st)
            if kind == "loop":
                loops.append((case, bow, con, ms, st))
    assert sum(st.n_scored < st.n_sharing for st in sts) * 2 >= len(sts)            # the 0.8 threshold bites
    assert sum(any(b != e and b in st.cand for _, b, e in st.acc_best) for st in sts) >= 3   # best != kf
    assert sum(len({b for a, b, _ in st.acc_best if a > np.float32(0.75) * st.bestAccScore}) <
               sum(a > np.float32(0.75) * st.bestAccScore for a, _, _ in st.acc_best) for st in sts) >= 2   # dedup
    assert sum(sum(a > np.float32(0.75) * st.bestAccScore for a, _, _ in st.acc_best) < st.n_score_and_match
               for st in sts) >= 1                                                      # retention drops entries
    # loop: an excluded keyframe would otherwise have been the best-scoring one
    excluded_best = 0
    for case, bow, con, ms, st in loops:
        bows = {}
        for s in case["steps"]:
            if s[0] == "add":
                bows[s[1]] = s[2]
            elif s[0] == "add_batch":
                bows.update(zip(s[1], s[2]))
        ql = (bow[0].tolist(), bow[1].tolist())
        sc = {k: np.float32(kr.l1_score(ql, (b[0].tolist(), b[1].tolist()))) for k, b in bows.items()}
        top = max(sc, key=sc.get)
        excluded_best += top in con and all(sc[top] > x for x in st.scored_score)
    assert excluded_best >= 2
    # loop: minScore removes scored entries that still contribute as neighbours
    contributes = 0
    for case, bow, con, ms, st in loops:
        below = {i for i, s in zip(st.scored_id, st.scored_score) if not s >= np.float32(ms)}
        cov = {s[1]: s[2] for s in case["steps"] if s[0] == "cov"}
        contributes += any(below & set(cov.get(e, [])[:10]) for _, _, e in st.acc_best)
    assert contributes >= 1


def _case(results, name):
    return results[name][1]


def test_boundary_words_equal_minCommonWords_is_not_scored(results):
    for st in _case(results, "words_eq_minCommonWords"):
        assert (st.n_sharing, st.maxCommonWords, st.minCommonWords) == (3, 10, 8)
        assert st.scored_id == [1, 3] and st.scored_words == [10, 9]     # keyframe 2 shares exactly 8
        assert 2 not in st.cand


def test_boundary_score_equal_minScore_is_kept(results):
    a, b, c = _case(results, "si_eq_minScore")
    assert a.scored_score == [np.float32(1.0), np.float32(0.75)]
    assert a.cand == [1] and np.isnan(a.scored_acc[1]) and a.n_score_and_match == 1     # si == minScore == 1
    assert b.n_score_and_match == 2 and b.scored_acc[1] == np.float32(0.75)             # si == minScore == 0.75
    assert c.n_score_and_match == 2


def test_boundary_acc_equal_retention_threshold_is_dropped(results):
    for st in _case(results, "acc_eq_retain"):
        assert st.scored_score == [np.float32(1.0), np.float32(0.75), np.float32(0.8125)]
        assert st.bestAccScore == np.float32(1.0) and st.n_score_and_match == 3
        assert st.cand == [1, 3]                                          # 0.75 == 0.75f * 1.0: not kept


def test_boundary_equal_neighbours_first_stays_best(results):
    a, b, c = _case(results, "equal_neighbours")
    for st in (a, b):
        assert st.scored_score == [np.float32(0.625), np.float32(0.75), np.float32(0.75)]
        assert st.acc_best[0] == (np.float32(2.125), 3, 1)                # covisibles [3, 2]: 3 comes first
        assert st.cand == [3]
    assert c.acc_best[0] == (np.float32(2.125), 2, 1) and c.cand == [2]   # covisibles [2, 3]
