#!/usr/bin/env python3
"""Time LocalMapping_KeyFrameCulling / LocalMapping_MapPointCulling on the map shape tools/map_timing.py uses
(tests/ba_cases.global_ba_problem: 2,000 keyframes, 4 laps of one circuit, 150 points created per keyframe).

  culling_timing.py [--reps R] [--out profiles/culling_timing.txt]

Every figure is the host time of one synchronous call with apply = 0 (argument staging, launches, downloads
and the wait included), median of R calls after one warm-up call, with the smallest and largest.  Recorded:
  * KeyFrameCulling over the covisibles of one keyframe with per-slot octaves drawn from 0-7, which leaves no
    candidate redundant (zero culls);
  * the same candidates after a handful of them got octave 7 in every slot and lost their points with fewer than
    ten observers, so that every observer of their points qualifies and they are culled;
  * the first such call after a mutation, which also uploads the key attributes and builds the cell index;
  * MapPointCulling of 4,000 points.
Absolute times only: no CPU baseline of LocalMapping::KeyFrameCulling exists in this repository."""
import argparse
import sys
import time
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, ".")
sys.path.insert(0, str(HERE.parent / "tests"))
import numpy as np  # noqa: E402

NKF, LAPS, PPK, FORCED = 2000, 4, 150, 6


def med(ts):
    return f"median {1e3 * np.median(ts):.3f}  min {1e3 * min(ts):.3f}  max {1e3 * max(ts):.3f} ms"


def timed(fn, reps):
    out, ts = None, []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return out, ts[1:], ts[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch  # noqa: F401  (its HIP runtime first, as the tests and the bench load it)
    import c_orb_slam_amd as orb
    from ba_cases import global_ba_problem
    pr = global_ba_problem(0, n_kf=NKF, pts_per_kf=PPK, laps=LAPS)
    pe, ke = pr["edge_pt"], pr["edge_kf"]
    npt = len(pr["pt_pos"])
    order = np.argsort(ke, kind="stable")
    start = np.searchsorted(ke[order], np.arange(NKF + 1))
    rows = [pe[order[start[k]:start[k + 1]]].astype(np.int32) for k in range(NKF)]
    rng = np.random.default_rng(2)
    mp = orb.Map()
    for k, r in enumerate(rows):
        mp.AddKeyFrame(k, r)
        mp.SetKeyFrameKeys(k, rng.integers(0, 8, len(r)).astype(np.uint8))
    cur = NKF // 2
    cand = mp.UpdateConnections(cur, cap_counter=NKF, cap_ordered=NKF)[2]
    nkf_, nslot, nobs = mp.size()
    lines = [f"# tools/culling_timing.py --reps {a.reps}  (MI355X; host time of one synchronous call, apply = 0; medians "
             f"after one warm-up call)",
             f"# map: global_ba_problem(0, n_kf={NKF}, pts_per_kf={PPK}, laps={LAPS}): {nkf_} keyframes, {nslot} row slots, "
             f"{nobs} observations, {npt} map points; candidates: the {len(cand)} covisibles of keyframe {cur}, rows of "
             f"{np.mean([len(rows[c]) for c in cand]):.0f} slots on average",
             "# no CPU baseline of LocalMapping::KeyFrameCulling / MapPointCulling exists here: absolute times only"]
    cull = lambda: mp.KeyFrameCulling(cand, None, True, apply=False, cap_bad=4096)
    mp.SetMapPointMatches(0, [0], [int(rows[0][0])], [1])                  # a mutation: the next call rebuilds
    g, ts, first = timed(cull, a.reps)
    lines.append(f"KeyFrameCulling, octaves 0-7 at random: {int((g['verdict'] == 1).sum())} culls, nRedundant / nMPs at most "
                 f"{max(r / max(m, 1) for r, m in zip(g['nRedundant'], g['nMPs'])):.2f}: {med(ts)}; the first call after "
                 f"a mutation (key upload + cell index over {nobs} observations + the row index rebuild): {1e3 * first:.3f} ms")
    seen_by = np.bincount(pe, minlength=npt)
    for c in cand[1:2 * FORCED:2]:
        few = np.nonzero(seen_by[rows[c]] < 4 + FORCED)[0].astype(np.int32)
        mp.SetMapPointMatches(int(c), few, np.full(len(few), -1, np.int32))
        mp.SetKeyFrameKeys(int(c), np.full(len(rows[c]), 7, np.uint8))
    g, ts, first = timed(cull, a.reps)
    lines.append(f"KeyFrameCulling, {FORCED} candidates with octave 7 everywhere and only points of 10 or more observers: "
                 f"{int((g['verdict'] == 1).sum())} culls, {len(g['bad_mp'])} points went bad: {med(ts)}; the first call after those mutations (key upload + "
                 f"cell index + the row index rebuild): {1e3 * first:.3f} ms")
    n = 4000
    pts = rng.permutation(npt)[:n].astype(np.int32)
    vis = rng.integers(1, 40, n).astype(np.int32)
    fnd = (vis * rng.choice([0.1, 0.3, 1.0], n)).astype(np.int32)
    fkf = (cur - rng.integers(0, 5, n)).astype(np.int32)
    (v, ob), ts, _ = timed(lambda: mp.MapPointCulling(pts, fkf, fnd, vis, cur, True, apply=False), a.reps)
    lines.append(f"MapPointCulling of {n} points (verdicts 0-4: {np.bincount(v, minlength=5).tolist()}): {med(ts)}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
