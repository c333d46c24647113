"""GPU: KeyFrameDatabase against the restatement tests/kfdb_ref.py.  Every comparison is by bit
pattern: ids, counts, float32 scores viewed as uint32 (NaN equal to NaN in scored_acc).

Reference: src/KeyFrameDatabase.cc (add 39-45, erase 47-67, clear 69-73, DetectLoopCandidates
76-197, DetectRelocalizationCandidates 199-309)."""
import ctypes as C
import threading

import numpy as np
import pytest

import kfdb_cases as kc
import kfdb_ref as kr
import vocab_cases as vc
import c_orb_slam_amd as orb
from c_orb_slam_amd import BowVector
from c_orb_slam_amd._lib import (ORB_E_CAPACITY, ORB_E_INVALID, ORB_OK, lib, orb_kfdb_query, orb_kfdb_result, ptr)

pytestmark = pytest.mark.gpu

CASES = {c["name"]: c for c in kc.gpu_cases()}


@pytest.fixture(scope="module")
def vocs(tmp_path_factory, gpu):
    d = tmp_path_factory.mktemp("kfdb_voc")
    out = {}
    for key, kw in (("small", kc.VOCAB), ("big", kc.VOCAB_BIG)):
        p = d / f"{key}.txt"
        leaves = vc.make_vocab(p, seed=3, stop_frac=0.0, trailing_newline=False, **kw)
        v = orb.ORBVocabulary()
        assert v.loadFromTextFile(p)
        assert v.info()["words"] == kc.n_words(kw)
        out[key] = (v, leaves)
    return out


def _voc(vocs, case):
    return vocs["big" if case["vocab"] is kc.VOCAB_BIG else "small"][0]


@pytest.fixture(scope="module")
def ref():
    """The restatement's stages of every case, computed once and shared."""
    return {n: kr.run_steps(c["steps"], kc.n_words(c["vocab"])) for n, c in CASES.items()}


def bv(b):
    return BowVector(b[0], b[1])


def run_gpu(db, steps):
    out = []
    for s in steps:
        op = s[0]
        if op == "add":
            db.add(s[1], bv(s[2]))
        elif op == "add_batch":
            db.add_batch(s[1], [bv(b) for b in s[2]])
        elif op == "erase":
            db.erase(s[1])
        elif op == "clear":
            db.clear()
        elif op == "cov":
            db.set_covisibles(s[1], s[2])
        elif op == "loop":
            out.append(db.DetectLoopCandidates(bv(s[1]), s[2], s[3], stages=True))
        elif op == "reloc":
            out.append(db.DetectRelocalizationCandidates(bv(s[1]), stages=True))
        elif op == "reloc_batch":
            out.append(db.DetectRelocalizationCandidates_batch([bv(b) for b in s[1]], stages=True))
    return out


def bits(a):
    a = np.asarray(a, np.float32)
    return np.where(np.isnan(a), np.uint32(0x7fc00000), a.view(np.uint32))


def same(got, st, what=""):
    """One query: library (candidates, stages) against the restatement's stages."""
    cand, g = got
    assert cand.tolist() == st.cand, what
    assert (g.n_sharing, g.maxCommonWords, g.minCommonWords, g.n_scored) == \
        (st.n_sharing, st.maxCommonWords, st.minCommonWords, st.n_scored), what
    assert g.scored_id.tolist() == st.scored_id, what
    assert g.scored_words.tolist() == st.scored_words, what
    assert np.array_equal(bits(g.scored_score), bits(st.scored_score)), what
    assert np.array_equal(bits(g.scored_acc), bits(st.scored_acc)), what
    assert bits([g.bestAccScore])[0] == bits([st.bestAccScore])[0], what


def same_all(got, want, what=""):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        if isinstance(w, list):
            assert len(g) == len(w)
            for j, (gg, ww) in enumerate(zip(g, w)):
                same(gg, ww, f"{what} query {i}.{j}")
        else:
            same(g, w, f"{what} query {i}")


def same_gpu(a, b):
    """Two library results, bit for bit."""
    assert a[0].tolist() == b[0].tolist()
    for f in ("n_sharing", "maxCommonWords", "minCommonWords", "n_scored"):
        assert getattr(a[1], f) == getattr(b[1], f), f
    for f in ("scored_id", "scored_words"):
        assert getattr(a[1], f).tolist() == getattr(b[1], f).tolist(), f
    for f in ("scored_score", "scored_acc"):
        assert np.array_equal(bits(getattr(a[1], f)), bits(getattr(b[1], f))), f
    assert bits([a[1].bestAccScore])[0] == bits([b[1].bestAccScore])[0]


@pytest.mark.parametrize("name", list(CASES))
def test_case_matches_restatement(vocs, ref, name):
    """Both Detect calls, candidates and every stage output, on the normal, boundary, lifecycle and
    batch cases: database sizes 1, 63, 64, 65, 300; BowVector lengths 1, 63, 64, 65, ~300, 4096."""
    case = CASES[name]
    db = orb.KeyFrameDatabase(_voc(vocs, case))
    same_all(run_gpu(db, case["steps"]), ref[name], name)


def test_batch_equals_single_calls(vocs):
    case = CASES["batch"]
    db = orb.KeyFrameDatabase(_voc(vocs, case))
    run_gpu(db, [s for s in case["steps"] if s[0] in ("cov", "add_batch")])
    sizes = []
    for s in case["steps"]:
        if s[0] != "reloc_batch":
            continue
        sizes.append(len(s[1]))
        got = db.DetectRelocalizationCandidates_batch([bv(b) for b in s[1]], stages=True)
        assert len(got) == len(s[1])
        for g, b in zip(got, s[1]):
            same_gpu(g, db.DetectRelocalizationCandidates(bv(b), stages=True))
            if len(b[0]) == 0:
                assert len(g[0]) == 0 and g[1].n_sharing == 0
    assert sizes == [1, 2, 7, 3]
    assert db.DetectRelocalizationCandidates_batch([]) == []


def test_empty_query_and_empty_database(vocs):
    db = orb.KeyFrameDatabase(vocs["small"][0])
    q = bv(CASES["kf24_len120"]["steps"][-2][1])
    empty = BowVector(np.zeros(0, np.uint32), np.zeros(0))
    assert db.size() == (0, 0)
    for cand, st in (db.DetectRelocalizationCandidates(q, stages=True),
                     db.DetectLoopCandidates(q, [], 0.1, stages=True)):
        assert len(cand) == 0 and (st.n_sharing, st.n_scored, st.maxCommonWords) == (0, 0, 0)
    run_gpu(db, CASES["kf24_len120"]["steps"][:-2])
    assert len(db.DetectRelocalizationCandidates(q)) >= 1
    for cand, st in (db.DetectRelocalizationCandidates(empty, stages=True),
                     db.DetectLoopCandidates(empty, [0], 0.1, stages=True)):
        assert len(cand) == 0 and (st.n_sharing, st.n_scored, st.maxCommonWords) == (0, 0, 0)


def test_add_one_at_a_time_equals_add_batch(vocs):
    case = CASES["kf48_len200"]
    loads = [s for s in case["steps"] if s[0] in ("cov", "add_batch")]
    queries = [s for s in case["steps"] if s[0] in ("loop", "reloc")]
    a = orb.KeyFrameDatabase(vocs["small"][0])
    b = orb.KeyFrameDatabase(vocs["small"][0])
    run_gpu(a, loads)
    for s in loads:
        if s[0] == "add_batch":
            for i, w in zip(s[1], s[2]):
                b.add(i, bv(w))
        else:
            run_gpu(b, [s])
    assert a.size() == b.size() == (48, sum(len(w[0]) for w in loads[-1][2]))
    for x, y in zip(run_gpu(a, queries), run_gpu(b, queries)):
        same_gpu(x, y)


def test_duplicate_add_and_absent_erase(vocs):
    case = CASES["kf24_len120"]
    db = orb.KeyFrameDatabase(vocs["small"][0])
    run_gpu(db, case["steps"][:-2])
    q = case["steps"][-2]
    before = run_gpu(db, [q])[0]
    size = db.size()
    other = bv(case["steps"][-1][1])
    with pytest.raises(orb.OrbGpuError) as ei:
        db.add(3, other)                                   # id 3 is present
    assert ei.value.code == ORB_E_INVALID
    with pytest.raises(orb.OrbGpuError) as ei:
        db.add_batch([500, 3], [other, other])             # all or none
    assert ei.value.code == ORB_E_INVALID
    with pytest.raises(orb.OrbGpuError) as ei:
        db.add_batch([500, 500], [other, other])
    assert ei.value.code == ORB_E_INVALID
    db.erase(kc.ABSENT + 9)                                # ORB_OK, nothing happens
    assert db.size() == size
    same_gpu(run_gpu(db, [q])[0], before)


def test_growth_and_compaction(vocs):
    """Initial capacity of 4 keyframes / 256 entries: 65 adds grow both tables, 40 erases leave more
    holes than live entries and compact the pool.  After each phase the database answers as a fresh
    one loaded by add_batch of the survivors in their sequence order, and as the restatement."""
    L = lib()
    W = kc.world(51, 65, 40, nplaces=3)
    rng = W["rng"]
    ids, bows = W["ids"], W["bows"]
    covs = [("cov", k, c) for k, c in W["covs"].items()]
    queries = [kc.reloc_step(W, 2), kc.loop_step(W, 30), kc.reloc_step(W, 64)]
    gone = set(rng.choice(65, size=40, replace=False).tolist())
    keep = [j for j in range(65) if j not in gone]
    assert L.orbgpu_unit_set_kfdb_initial_capacity(4, 256) == 0
    try:
        db = orb.KeyFrameDatabase(vocs["small"][0])
    finally:
        assert L.orbgpu_unit_set_kfdb_initial_capacity(0, 0) == 0
    run_gpu(db, covs)
    for j in range(65):
        db.add(ids[j], bv(bows[j]))
        if j in (3, 4, 5, 31):                             # around the first doublings
            assert len(db.DetectRelocalizationCandidates(bv(bows[j]))) >= 1
    assert db.size() == (65, sum(len(b[0]) for b in bows))
    full = run_gpu(db, queries)
    for j in sorted(gone):
        db.erase(ids[j])
    assert db.size() == (25, sum(len(bows[j][0]) for j in keep))
    part = run_gpu(db, queries)
    db.add(ids[min(gone)], bv(bows[min(gone)]))            # a freed slot is taken again
    again = run_gpu(db, queries)
    for have, idx in ((full, list(range(65))), (part, keep), (again, keep + [min(gone)])):
        fresh = orb.KeyFrameDatabase(vocs["small"][0])
        load = covs + [("add_batch", [ids[j] for j in idx], [bows[j] for j in idx])]
        run_gpu(fresh, load)
        for x, y in zip(have, run_gpu(fresh, queries)):
            same_gpu(x, y)
        same_all(have, kr.run_steps(load + queries, W["nw"]))


def _raw(bow, cap, cap_scored, ex=None, minScore=0.0):
    w, v = np.ascontiguousarray(bow[0], np.uint32), np.ascontiguousarray(bow[1], np.float64)
    ex = np.ascontiguousarray(ex if ex is not None else [], np.int32)
    bufs = dict(w=w, v=v, ex=ex, cand=np.full(cap + 4, -7, np.int32), id=np.full(cap_scored + 4, -7, np.int32),
                words=np.full(cap_scored + 4, -7, np.int32), score=np.full(cap_scored + 4, -7, np.float32),
                acc=np.full(cap_scored + 4, -7, np.float32))
    q = orb_kfdb_query(len(w), ptr(w), ptr(v), len(ex), ptr(ex) if len(ex) else None, minScore)
    r = orb_kfdb_result(cap, ptr(bufs["cand"]), 0, cap_scored, ptr(bufs["id"]), ptr(bufs["words"]), ptr(bufs["score"]),
                        ptr(bufs["acc"]), 0, 0, 0, 0, 0.0)
    return q, r, bufs


def test_errors_that_need_a_handle(vocs, ref, tmp_path):
    L = lib()
    name = "kf300_len300"
    case = CASES[name]
    db = orb.KeyFrameDatabase(vocs["small"][0])
    run_gpu(db, case["steps"][:-2])
    # a word id >= the vocabulary's word count
    bad = BowVector([5, 999, 1000], [0.5, 0.25, 0.25])
    size = db.size()
    with pytest.raises(orb.OrbGpuError) as ei:
        db.add(4000, bad)
    assert ei.value.code == ORB_E_INVALID and db.size() == size
    for call in (lambda: db.DetectRelocalizationCandidates(bad), lambda: db.DetectLoopCandidates(bad, [], 0.0)):
        with pytest.raises(orb.OrbGpuError) as ei:
            call()
        assert ei.value.code == ORB_E_INVALID
    # capacity: the needed counts come back, nothing is written past the capacities, a retry succeeds
    for step, st in zip(case["steps"][-2:], ref[name]):
        assert len(st.cand) >= 2 and st.n_scored >= 3
        ex, ms = (step[2], step[3]) if step[0] == "loop" else (None, 0.0)
        fn = L.KeyFrameDatabase_DetectLoopCandidates if step[0] == "loop" else \
            L.KeyFrameDatabase_DetectRelocalizationCandidates
        q, r, b = _raw(step[1], 1, 2, ex, ms)
        assert fn(db._h, C.byref(q), C.byref(r)) == ORB_E_CAPACITY
        assert (r.n_cand, r.n_scored) == (len(st.cand), st.n_scored)
        assert b["cand"][0] == st.cand[0] and (b["cand"][1:] == -7).all()
        assert b["id"][:2].tolist() == st.scored_id[:2]
        for k in ("id", "words", "score", "acc"):
            assert (b[k][2:] == -7).all(), k
        q, r, b = _raw(step[1], r.n_cand, r.n_scored, ex, ms)
        assert fn(db._h, C.byref(q), C.byref(r)) == ORB_OK
        assert b["cand"][:r.n_cand].tolist() == st.cand and (b["cand"][r.n_cand:] == -7).all()
        assert b["id"][:r.n_scored].tolist() == st.scored_id and (b["id"][r.n_scored:] == -7).all()
        # candidates alone: no stage buffers, any number scored
        q, r, b = _raw(step[1], len(st.cand), 0, ex, ms)
        r.scored_id = r.scored_words = r.scored_score = r.scored_acc = None
        assert fn(db._h, C.byref(q), C.byref(r)) == ORB_OK and r.n_scored == st.n_scored
    # a non-L1 vocabulary
    p = tmp_path / "l2.txt"
    vc.make_vocab(p, k=10, L=2, seed=4, scoring=1)
    v2 = orb.ORBVocabulary()
    assert v2.loadFromTextFile(p)
    db2 = orb.KeyFrameDatabase(v2)
    ok = BowVector([1, 2], [0.5, 0.5])
    for call in (lambda: db2.DetectRelocalizationCandidates(ok), lambda: db2.DetectLoopCandidates(ok, [], 0.0),
                 lambda: db2.DetectRelocalizationCandidates_batch([ok, ok])):
        with pytest.raises(orb.OrbGpuError) as ei:
            call()
        assert ei.value.code == ORB_E_INVALID


def test_end_to_end_with_the_vocabulary_transform(vocs):
    """BowVectors as ORBVocabulary.transform makes them (ascending words, double values) go into add
    and query; the result equals the restatement fed with the same vectors."""
    voc, leaves = vocs["small"]
    rng = np.random.default_rng(61)
    places = [rng.choice(len(leaves), size=150, replace=False) for _ in range(3)]
    bows, place = [], []
    for i in range(30):
        p = i % 3
        bow, _ = voc.transform(vc.features_near(leaves[places[p]], 400, seed=100 + i, noise_bits=6))
        bows.append((bow.words, bow.values))
        place.append(p)
    assert all(len(b[0]) > 20 for b in bows)
    ids = list(range(10, 40))
    steps = [("cov", ids[i], [ids[j] for j in range(30) if place[j] == place[i] and j != i][:10]) for i in range(30)]
    steps += [("add", ids[i], bows[i]) for i in range(30)]
    for p in range(3):
        qb, _ = voc.transform(vc.features_near(leaves[places[p]], 400, seed=900 + p, noise_bits=6))
        steps.append(("reloc", (qb.words, qb.values)))
        con = [ids[p], ids[p + 3]]
        ms = min(kr.l1_score((qb.words.tolist(), qb.values.tolist()), (bows[j][0].tolist(), bows[j][1].tolist()))
                 for j in (p, p + 3))
        steps.append(("loop", (qb.words, qb.values), con, float(np.float32(ms))))
    want = kr.run_steps(steps, kc.n_words(kc.VOCAB))
    assert all(len(st.cand) >= 1 for st in want[::2])
    db = orb.KeyFrameDatabase(voc)
    same_all(run_gpu(db, steps), want, "end to end")


def test_two_host_threads_query_one_handle(vocs, ref):
    name = "kf65_len64"
    case = CASES[name]
    db = orb.KeyFrameDatabase(_voc(vocs, case))
    run_gpu(db, case["steps"][:-2])
    reloc, loop = case["steps"][-2:]
    seq = run_gpu(db, [reloc, loop])
    same_all(seq, ref[name], name)
    got = {0: [], 1: []}
    errs = []

    def work(t, step):
        try:
            for _ in range(20):
                got[t] += run_gpu(db, [step])
        except Exception as e:   # noqa: BLE001
            errs.append(e)

    th = [threading.Thread(target=work, args=(0, reloc)), threading.Thread(target=work, args=(1, loop))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    assert len(got[0]) == len(got[1]) == 20
    for t in (0, 1):
        for g in got[t]:
            same_gpu(g, seq[t])


def test_timings_are_reported(vocs):
    case = CASES["kf24_len120"]
    db = orb.KeyFrameDatabase(vocs["small"][0])
    run_gpu(db, case["steps"][:-2])
    db.enable_timing(True)
    run_gpu(db, case["steps"][-2:-1])
    ms = db.last_timings()
    assert np.isfinite(ms).all() and (ms >= 0).all() and ms[2] > 0
