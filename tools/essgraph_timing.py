#!/usr/bin/env python3
"""Time Optimizer_OptimizeEssentialGraph on a loop-closed 4-lap ring (the global-BA workload's map
just before global BA): N keyframes on `laps` laps of a circle, parent edges i -> i-1, covisibility
edges to the previous 2-3 keyframes and to the keyframe one lap earlier, stored loop edges at the
lap joins, LoopConnections edges from the corrected keyframes to keyframes 0 and 1.

  essgraph_timing.py [N] [--laps L] [--reps R] [--free-scale]    ms per call (the call returns after
                                                                  its stream is drained: host clock)
  essgraph_timing.py --stats <*_kernel_stats.csv>                 kernel split of a separate
      rocprofv3 --kernel-trace --stats -f csv -d DIR -o ess -- python3 tools/essgraph_timing.py --reps 2

Run it from the repository root: the graph is built with the Sim3 helpers of
tests/essgraph_cases.py, so tests/ is put on sys.path.
"""
import argparse
import csv
import sys
import time

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import numpy as np  # noqa: E402

GROUPS = (("linearisation", ("k_ess_lin", "k_ess_meas")), ("assembly", ("k_ess_assemble",)),
          ("solve", ("ldlt", "k_scal_pub", "k_fail_pub", "k_x_zero_rows")),
          ("update + sums", ("k_ess_update", "k_ess_sum")), ("finish", ("k_ess_finish", "k_ess_points")))


def lap_ring(N, laps, seed=0, fix_scale=True, n_corrected=4):
    import essgraph_cases as ec
    rng = np.random.default_rng(seed)
    per = N // laps
    a = 2 * np.pi * np.arange(N) / per
    Rwc = np.zeros((N, 3, 3))
    Rwc[:, 0, 0], Rwc[:, 0, 1], Rwc[:, 1, 0], Rwc[:, 1, 1], Rwc[:, 2, 2] = np.cos(a), -np.sin(a), np.sin(a), np.cos(a), 1
    c = np.stack([10 * np.cos(a), 10 * np.sin(a), 0.02 * (np.arange(N) // per)], -1)
    Rcw = np.swapaxes(Rwc, -1, -2)
    T = (Rcw, -(Rcw @ c[..., None])[..., 0], np.ones(N))
    u = np.concatenate([0.002 * rng.standard_normal((N, 3)), 0.01 * rng.standard_normal((N, 3)),
                        (0.0 if fix_scale else 0.002) * rng.standard_normal((N, 1))], -1)
    D = ec.s3_exp(u)
    one = lambda S, k: (S[0][k], S[1][k], S[2][k])   # noqa: E731
    S = [one(T, 0)]
    for k in range(1, N):
        S.append(ec.mul(one(D, k), ec.mul(ec.mul(one(T, k), ec.inv(one(T, k - 1))), S[-1])))
    corrected = list(range(N - n_corrected, N))
    Scw = list(S)
    for k in corrected:
        Scw[k] = ec.mul(ec.mul(S[k], ec.inv(S[N - 1])), one(T, N - 1))
    loop = [(k, j) for k in corrected for j in (0, 1)]
    joined = {frozenset(p) for p in loop}
    normal = []
    for i in range(1, N):
        for j in (i - 1, i - 2, i - 3, i - per, i - per - 1):
            if j >= 0 and frozenset((i, j)) not in joined:
                normal.append((i, j))
        if i % per == 0:
            normal.append((i, 0))   # the loop edge an earlier closure stored at this lap join
    stack = lambda L: (np.stack([x[0] for x in L]), np.stack([x[1] for x in L]), np.array([x[2] for x in L]))   # noqa: E731
    edges = loop + normal
    fixed = np.zeros(N, np.uint8)
    fixed[0] = 1
    mp = (10 * rng.standard_normal((50 * N, 3))).astype(np.float32)
    return dict(Scw=ec.sim3_to_rows(stack(Scw)), ScwNonCorrected=ec.sim3_to_rows(stack(S)), fixed=fixed,
                edge_i=np.array([e[0] for e in edges], np.int32), edge_j=np.array([e[1] for e in edges], np.int32),
                edge_loop=np.array([1] * len(loop) + [0] * len(normal), np.uint8), bFixScale=int(fix_scale),
                mp_pos=mp, mp_ref=rng.integers(0, N, len(mp)).astype(np.int32))


def stats(path):
    rows = list(csv.DictReader(open(path)))
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    print(f"{'group':16s} {'launches':>9s} {'total_ms':>10s} {'share':>7s}")
    left = rows
    for name, keys in GROUPS + (("other (fills)", None),):
        sel = left if keys is None else [r for r in left if any(k in r["Name"] for k in keys)]
        left = [r for r in left if r not in sel]
        ns = sum(float(r["TotalDurationNs"]) for r in sel)
        print(f"{name:16s} {sum(int(r['Calls']) for r in sel):9d} {ns / 1e6:10.3f} {100 * ns / max(total, 1):6.1f}%")
    print(f"{'kernels total':16s} {sum(int(r['Calls']) for r in rows):9d} {total / 1e6:10.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("N", nargs="?", type=int, default=2000)
    ap.add_argument("--laps", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--free-scale", action="store_true")
    ap.add_argument("--stats")
    a = ap.parse_args()
    if a.stats:
        return stats(a.stats)
    from c_orb_slam_amd import OptimizeEssentialGraph
    pr = lap_ring(a.N, a.laps, fix_scale=not a.free_scale)
    out = OptimizeEssentialGraph(pr, 20)   # warm-up: arena, symbolic factorisation caches, code objects
    ts = []
    for _ in range(a.reps):
        t = time.perf_counter()
        out = OptimizeEssentialGraph(pr, 20)
        ts.append(time.perf_counter() - t)
    print(f"N={a.N} laps={a.laps} edges={len(pr['edge_i'])} rows={7 * (a.N - 1)} map points={len(pr['mp_ref'])} "
          f"scale {'free' if a.free_scale else 'fixed'}")
    print(f"chi2 {out['chi2'][0]:.6g} -> {out['chi2'][-1]:.6g}, {out['n_solves']} LM iterations, "
          f"{out['lm_trials']} factorisations")
    print(f"ms per call: median {1e3 * np.median(ts):.2f}  min {1e3 * min(ts):.2f}  max {1e3 * max(ts):.2f}  "
          f"({a.reps} calls after one warm-up; includes the host list build, the nested dissection and the upload)")


if __name__ == "__main__":
    main()
