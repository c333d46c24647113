#!/usr/bin/env python3
"""Time LocalMapping_CreateNewMapPoints_batch and MapPoint_Update_batch: ms per call by a host
clock around the synchronous C calls (the argument structures are built once, outside the
clock), after a warm-up.

  localmap_timing.py [--reps R]      10 and 20 neighbours x 300 pairs; an update of 2,000 points
                                     with 2..60 observations each and a few with 300
  localmap_timing.py --stats <*_kernel_stats.csv>     kernel split of a separate
      rocprofv3 --kernel-trace --stats -f csv -d DIR -o lm -- python3 tools/localmap_timing.py --reps 2

Run it from the repository root: the scenes come from tests/localmap_cases.py.
"""
import argparse
import csv
import ctypes as C
import sys
import time

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import numpy as np  # noqa: E402


def stats(path):
    rows = list(csv.DictReader(open(path)))
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    print(f"{'kernel':28s} {'launches':>9s} {'total_ms':>10s} {'avg_us':>9s} {'share':>7s}")
    for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"])):
        ns, calls = float(r["TotalDurationNs"]), int(r["Calls"])
        print(f"{r['Name'].split('(')[0][-28:]:28s} {calls:9d} {ns / 1e6:10.3f} {ns / 1e3 / max(calls, 1):9.1f} "
              f"{100 * ns / max(total, 1):6.1f}%")


def timed(fn, reps):
    fn()                                   # warm-up: arena growth, code object load
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return f"median {1e3 * np.median(ts):.3f}  min {1e3 * min(ts):.3f}  max {1e3 * max(ts):.3f} ms"


def triangulation_call(m, L, n_neigh, npairs, stereo_frac=0.5):
    import localmap_cases as lc
    from c_orb_slam_amd._lib import orb_triangulate, ptr
    base, nbs = lc.multi_scene("sideways", stereo_frac, [npairs] * n_neigh)
    k1 = base["KF1"].cstruct()
    arr = (orb_triangulate * n_neigh)()
    keep, outs = [base, nbs], []       # the structures hold raw pointers into these arrays
    for j, (KF2, d2, s2, pr) in enumerate(nbs):
        k2 = KF2.cstruct()
        out = [np.zeros((npairs, 3), np.float32), np.zeros(npairs, np.int8), np.zeros((npairs, 3), np.float32),
               np.zeros(npairs, np.float32), np.zeros(npairs, np.float32)]
        keep.append(k2)
        outs.append(out)
        q = arr[j]
        q.KF2, q.depth2, q.levelSigma2_2, q.npairs, q.pairs = C.pointer(k2), ptr(d2), ptr(s2), npairs, ptr(pr)
        q.x3D, q.status, q.normal, q.max_dist, q.min_dist = (ptr(a) for a in out)
    d1, s1 = base["depth1"], base["sigma2"]

    def call():
        rc = L.LocalMapping_CreateNewMapPoints_batch(m._h, C.byref(k1), ptr(d1), ptr(s1), 1.2, n_neigh, arr)
        assert rc == 0, rc
    call.keep = keep
    call.created = lambda: sum(int((o[1] > 0).sum()) for o in outs)
    return call


def update_call(m, L, npts=2000, seed=0):
    import localmap_cases as lc
    from c_orb_slam_amd._lib import orb_pointupdate, ptr
    rng = np.random.default_rng(seed)
    ks = rng.integers(2, 61, npts)
    ks[rng.choice(npts, 5, replace=False)] = 300
    c = lc.update_case([int(k) for k in ks])
    out = dict(best=np.zeros(npts, np.int32), normal=np.zeros((npts, 3), np.float32),
               max_dist=np.zeros(npts, np.float32), min_dist=np.zeros(npts, np.float32))
    U = orb_pointupdate()
    U.npts = npts
    for k, v in {**c, **out}.items():
        setattr(U, k, ptr(v))

    def call():
        rc = L.MapPoint_Update_batch(m._h, C.byref(U))
        assert rc == 0, rc
    call.keep = (c, out)
    call.total = int(ks.sum())
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--stats")
    a = ap.parse_args()
    if a.stats:
        return stats(a.stats)
    import c_orb_slam_amd as orb
    L = orb.lib()
    m = orb.ORBmatcher(0.6, True)
    for n_neigh in (10, 20):
        call = triangulation_call(m, L, n_neigh, 300)
        print(f"CreateNewMapPoints {n_neigh} neighbours x 300 pairs: {timed(call, a.reps)}  "
              f"({call.created()} of {300 * n_neigh} pairs created; {a.reps} calls after one warm-up)")
    call = update_call(m, L)
    print(f"MapPoint_Update 2000 points, {call.total} observations (2..60 each, five with 300): "
          f"{timed(call, a.reps)}")


if __name__ == "__main__":
    main()
