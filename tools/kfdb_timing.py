#!/usr/bin/env python3
"""Time the KeyFrameDatabase queries at 500 / 2,000 / 10,000 stored keyframes of about 1,000 words:
one DetectLoopCandidates, one DetectRelocalizationCandidates and one relocalization batch of 64,
each as ms per call by a host clock around the synchronous C call (arguments built once, outside the
clock) and, in a second set of calls, the three KeyFrameDatabase_last_timings figures (share count
and selection, scoring: HIP events on the handle's stream; whole call: the library's host clock).

  kfdb_timing.py [--reps R] [--out profiles/kfdb_timing.txt]

Run it from the repository root.  The vocabulary is a synthetic k = 10, L = 4 tree (10^4 words,
tests/vocab_cases.make_vocab); the keyframes come in 50 places whose members draw 85 % of their
words from a pool of 1,300.  ORBvoc.txt has 10^6 words, so real BowVectors share far more sparsely:
the scored share here (and with it the scoring time) is an upper bound.  There is no CPU baseline
of KeyFrameDatabase.cc in this repository, so no speed-up is claimed.
"""
import argparse
import sys
import tempfile
import time
from pathlib import Path

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import numpy as np  # noqa: E402

NW, BLEN, PLACES, POOL = 10000, 1000, 50, 1300


def bow(rng, pool):
    w = np.unique(np.concatenate([rng.choice(pool, size=int(BLEN * 0.85), replace=False),
                                  rng.integers(0, NW, BLEN - int(BLEN * 0.85))]).astype(np.uint32))
    v = rng.uniform(0.05, 1.0, len(w))
    return w, v / v.sum()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out")
    a = ap.parse_args()
    import vocab_cases as vc
    import c_orb_slam_amd as orb
    from c_orb_slam_amd import BowVector
    from c_orb_slam_amd._lib import lib, orb_kfdb_query, orb_kfdb_result, ptr
    L = lib()
    with tempfile.TemporaryDirectory() as d:
        p = Path(d) / "voc.txt"
        vc.make_vocab(p, k=10, L=4, seed=1, stop_frac=0.0, trailing_newline=False)
        voc = orb.ORBVocabulary()
        assert voc.loadFromTextFile(p) and voc.info()["words"] == NW
    lines = [f"# tools/kfdb_timing.py --reps {a.reps}  (MI355X; host clock around the synchronous C call; "
             "last_timings in a second pass; medians over the calls after one warm-up)",
             f"# vocabulary: synthetic k=10 L=4, {NW} words; keyframes of ~{BLEN} words in {PLACES} places "
             f"(pool {POOL}, 85 % from the pool).  ORBvoc.txt has 10^6 words: real vectors share far more sparsely, so the scored "
             "share and the scoring time here are an upper bound",
             "# no CPU baseline of KeyFrameDatabase.cc exists here: these are absolute times only"]
    for nkf in (500, 2000, 10000):
        rng = np.random.default_rng(nkf)
        pools = [rng.choice(NW, size=POOL, replace=False) for _ in range(PLACES)]
        place = rng.integers(0, PLACES, nkf)
        bows = [bow(rng, pools[pl]) for pl in place]
        db = orb.KeyFrameDatabase(voc)
        db.add_batch(np.arange(nkf), [BowVector(*b) for b in bows])
        for i in range(nkf):
            mates = np.flatnonzero(place == place[i])
            db.set_covisibles(i, rng.choice(mates, size=min(10, len(mates)), replace=False))
        nk, ne = db.size()
        qb = [bow(rng, pools[int(rng.integers(0, PLACES))]) for _ in range(64)]
        ex = np.ascontiguousarray(np.flatnonzero(place == place[0])[:20], np.int32)
        keep = []

        def args(n, loop):
            qs, rs = [], []
            for i in range(n):
                w, v = qb[i]
                cand, sid = np.zeros(1024, np.int32), np.zeros(nkf, np.int32)
                keep.append((cand, sid))
                qs.append(orb_kfdb_query(len(w), ptr(w), ptr(v), len(ex) if loop else 0, ptr(ex) if loop else None,
                                         0.05))
                rs.append(orb_kfdb_result(1024, ptr(cand), 0, nkf, ptr(sid), None, None, None, 0, 0, 0, 0, 0.0))
            return (orb_kfdb_query * n)(*qs), (orb_kfdb_result * n)(*rs)

        q1, r1 = args(1, True)
        q2, r2 = args(1, False)
        q3, r3 = args(64, False)
        calls = [("loop x1", lambda: L.KeyFrameDatabase_DetectLoopCandidates(db._h, q1, r1), r1),
                 ("reloc x1", lambda: L.KeyFrameDatabase_DetectRelocalizationCandidates(db._h, q2, r2), r2),
                 ("reloc x64", lambda: L.KeyFrameDatabase_DetectRelocalizationCandidates_batch(db._h, 64, q3, r3), r3)]
        lines.append(f"keyframes {nk} ({ne} entries)")
        for name, call, r in calls:
            db.enable_timing(False)
            assert call() == 0                # warm-up: buffer growth, code object load
            ts = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                rc = call()
                ts.append(time.perf_counter() - t0)
                assert rc == 0, rc
            db.enable_timing(True)
            assert call() == 0
            ks = []
            for _ in range(a.reps):
                assert call() == 0
                ks.append(db.last_timings().copy())
            k = np.median(np.array(ks), axis=0)
            nq = len(r)
            lines.append(f"  {name:9s}: call median {1e3 * np.median(ts):.3f}  min {1e3 * min(ts):.3f}  "
                         f"max {1e3 * max(ts):.3f} ms | last_timings (ms) share {k[0]:.3f}  scoring {k[1]:.3f}  "
                         f"whole {k[2]:.3f} | per query: sharing {np.mean([r[i].n_sharing for i in range(nq)]):.0f}  "
                         f"scored {np.mean([r[i].n_scored for i in range(nq)]):.0f}  "
                         f"candidates {np.mean([r[i].n_cand for i in range(nq)]):.1f}")
        db.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
