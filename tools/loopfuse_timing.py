#!/usr/bin/env python3
"""Time LoopClosing_SearchAndFuse on a loop-closure-sized workload: 25 corrected keyframes, 1,241 x 376 frames
at 2,000 features, 6,000 loop map points.

  loopfuse_timing.py [--reps R] [--keyframes K] [--out profiles/loopfuse_timing.txt]

It prints
  * the stage times of the call (projection, match and descriptor recomputation summed over the passes: HIP
    events; host replay: wall clock; LoopClosing_SearchAndFuse_last_timings) and the call's wall time,
    apply = 0 so that every repetition meets the same map;
  * for the same inputs, the library time of the exact route an adapter had before this entry: one
    ORBmatcher_Fuse_Sim3 per keyframe with one MapPoint_Update_batch between every two of them (and one after
    the "Start Loop Fusion" block) for the points that survived a Replace.  Only the time inside those
    library calls is summed; the replay between them runs in Python (tests/loopfuse_ref.py, the same
    mutations) and is not counted, although a real adapter pays for its own.
The two routes must end with the same op log; the tool checks that before it prints.

The scene is synthetic: world points in front of the loop-side camera, keyframes a small rotation and a few
centimetres away, keypoints = projections with 0.3 px of noise, descriptors = the point's with a few bits
flipped.  Three loop-side keyframes that are not listed observe the loop points.  Per listed keyframe and
feature the keyframe holds the loop point itself (30 %), a duplicate point (20 %) or nothing.  The Sim3 of a
keyframe is (q(R), s t, s), s cycling over 1, 0.93, 1.08, 0.97.  mvpCurrentMatchedPoints names the loop point
of half of the held slots of the highest keyframe and a loop point for 5 % of its empty ones.  No images are
extracted, so the keypoint distribution is uniform, not a KITTI one."""
import argparse
import sys
import time
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, ".")
sys.path.insert(0, str(HERE.parent / "tests"))
import numpy as np  # noqa: E402

W, H, NFEAT, NLOOP, NLOOPKF = 1241, 376, 2000, 6000, 3
SCALES = (1.0, 0.93, 1.08, 0.97)


def quat_of(R):
    w = np.sqrt(1.0 + R[0, 0] + R[1, 1] + R[2, 2]) / 2.0
    q = np.array([(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w])
    return q / np.linalg.norm(q)


def scene(nlisted, seed=0):
    import c_orb_slam_amd as orb
    from c_orb_slam_amd import synthetic
    from c_orb_slam_amd._lib import KP_DTYPE
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = synthetic.KITTI_K
    bf = synthetic.KITTI_BF
    scale = (np.float32(1.2) ** np.arange(8)).astype(np.float32)
    nw = NLOOP
    z = rng.uniform(8, 60, nw)
    X = np.stack([(rng.uniform(20, W - 20, nw) - cx) / fx * z, (rng.uniform(20, H - 20, nw) - cy) / fy * z, z], 1)
    base = rng.integers(0, 256, (nw, 32), dtype=np.uint8)
    octv = rng.integers(0, 6, nw)
    nkf = nlisted + NLOOPKF                              # listed: 0 .. nlisted - 1, loop side: the ids after them
    T, Ow = [], np.zeros((nkf, 3), np.float32)
    for k in range(nkf):
        R = np.eye(3) if k == nlisted else synthetic.small_rotation(rng, fx, max_shift=20.0)
        t = np.zeros(3) if k == nlisted else rng.normal(0, 0.05, 3)
        T.append(synthetic.pose_from_rotation(R, t))
        Ow[k] = -(R.T @ t)
    pos, desc, normal, maxd, mind = ([] for _ in range(5))

    def new_point(Xw, d, k, o):
        PC = Xw.astype(np.float32) - Ow[k]
        dist = np.float32(np.linalg.norm(PC))
        pos.append(Xw.astype(np.float32)); desc.append(d); normal.append(PC / dist)
        maxd.append(np.float32(dist * scale[o])); mind.append(np.float32(maxd[-1] / scale[-1]))
        return len(pos) - 1

    for p in range(nw):                                  # the loop points: rows 0 .. nw - 1
        new_point(X[p], base[p], nlisted, int(octv[p]))
    frames, rows = {}, {}
    for k in list(range(nlisted, nkf)) + list(range(nlisted)):
        Xc = X @ T[k][:3, :3].astype(np.float64).T + T[k][:3, 3].astype(np.float64)
        u, v = fx * Xc[:, 0] / Xc[:, 2] + cx, fy * Xc[:, 1] / Xc[:, 2] + cy
        vis = np.flatnonzero((u > 2) & (u < W - 2) & (v > 2) & (v < H - 2) & (Xc[:, 2] > 1))
        vis = rng.permutation(vis)[:NFEAT]
        n = len(vis)
        kp = np.zeros(n, KP_DTYPE)
        kp["x"], kp["y"] = u[vis] + rng.normal(0, 0.3, n), v[vis] + rng.normal(0, 0.3, n)
        kp["octave"], kp["size"] = octv[vis], 31
        d = base[vis].copy()
        for _ in range(3):
            d[np.arange(n), rng.integers(0, 32, n)] ^= np.uint8(1) << rng.integers(0, 8, n).astype(np.uint8)
        frames[k] = orb.Frame(kp, d, scale, T[k], fx, fy, cx, cy, bf, W, H)
        row = np.full(n, -1, np.int32)
        if k >= nlisted:
            row[:] = vis                                 # a loop-side keyframe observes the loop points it sees
        else:
            r = rng.random(n)
            for j in range(n):
                if r[j] < 0.3:
                    row[j] = vis[j]
                elif r[j] < 0.5:
                    row[j] = new_point(X[vis[j]], d[j].copy(), k, int(octv[vis[j]]))
        rows[k] = (row, vis)
    ops = []
    for k in range(nkf):
        ops.append(("AddKeyFrame", k, rows[k][0]))
        ops.append(("SetKeyFrameKeys", k, frames[k].keysUn["octave"].astype(np.uint8), None))
    n = len(pos)
    table = dict(pos=np.array(pos, np.float32).reshape(-1, 3), normal=np.array(normal, np.float32).reshape(-1, 3),
                 max_dist=np.array(maxd, np.float32), min_dist=np.array(mind, np.float32),
                 desc=np.array(desc, np.uint8).reshape(-1, 32), bad=np.zeros(n, np.uint8))
    kf = list(range(nlisted))
    Scw = np.zeros((nlisted, 8))
    for k in kf:
        s = SCALES[k % len(SCALES)]
        Tk = T[k].astype(np.float64)
        Scw[k] = np.concatenate([quat_of(Tk[:3, :3]), s * Tk[:3, 3], [s]])
    cur_kf = nlisted - 1
    row, vis = rows[cur_kf]
    matched = np.full(len(row), -1, np.int32)
    inrow = set(int(p) for p in row if p >= 0)
    pool = [p for p in rng.permutation(nw) if int(p) not in inrow]
    for j in range(len(row)):
        if row[j] >= 0 and rng.random() < 0.5:
            matched[j] = vis[j]                          # the slot's own point or the one its duplicate copies
        elif row[j] < 0 and rng.random() < 0.05 and int(vis[j]) not in inrow:
            matched[j] = pool.pop()
    kw = dict(kf=kf, frames=[frames[k] for k in kf], Scw=Scw, loop_pts=np.arange(nw, dtype=np.int32),
              kf_desc={k: frames[k].desc for k in range(nkf)}, logScaleFactor=np.float32(np.log(np.float32(1.2))),
              cur_kf=cur_kf, matched=matched, th=4.0, n_kf_rows=nkf)
    return dict(ops=ops, table=table, kw=kw)


def fill(target, ops):
    for op in ops:
        getattr(target, op[0])(*op[1:])
    return target


def parent_route(m, s):
    """-> (seconds inside ORBmatcher_Fuse_Sim3 and inside MapPoint_Update_batch with the calls of each, the result)"""
    import loopfuse_ref
    from culling_ref import CullRefMap
    spent = dict(fuse=0.0, update=0.0, nfuse=0, nupdate=0)

    def timed_fuse(KF, Scw, pts, geo, skip, lsf, th):
        t0 = time.perf_counter()
        out = m.Fuse_Sim3(KF, Scw, pts, geo, skip, lsf, th)
        spent["fuse"] += time.perf_counter() - t0
        spent["nfuse"] += 1
        return out

    class Route(loopfuse_ref.SearchAndFuseRef):
        pending = None

        def ComputeDistinctiveDescriptors(self, p):
            if not self.isBad(p):
                obs = self._observations(p)
                if obs:
                    self.pending[p] = np.stack([self.kf_desc[kf.mnId][idx] for kf, idx in obs])
            super().ComputeDistinctiveDescriptors(p)

        def flush(self):
            rows = list(self.pending.values())
            self.pending = {}
            if not rows:
                return
            start = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
            t0 = time.perf_counter()
            m.UpdateMapPoints(start, obs_desc=np.concatenate(rows))
            spent["update"] += time.perf_counter() - t0
            spent["nupdate"] += 1

        def step0(self):
            super().step0()
            self.flush()

        def Fuse(self, *a):
            n = super().Fuse(*a)
            self.flush()
            return n

    saved = loopfuse_ref.oracle_lib.oracle_fuse_sim3
    loopfuse_ref.oracle_lib.oracle_fuse_sim3 = timed_fuse
    try:
        r = Route(fill(CullRefMap(), s["ops"]), table=s["table"], **s["kw"])
        r.pending = {}
        r.run()
    finally:
        loopfuse_ref.oracle_lib.oracle_fuse_sim3 = saved
    return spent, r.result()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--keyframes", type=int, default=25)
    ap.add_argument("--out")
    a = ap.parse_args()
    import c_orb_slam_amd as orb
    assert orb.device_available(), "loopfuse_timing.py needs a HIP device"
    s = scene(a.keyframes)
    m = orb.ORBmatcher(0.6, True)
    mp = fill(orb.Map(), s["ops"])
    mp.enable_timing(True)
    lcl = orb.LoopClosing(m, mp)
    walls, stages, got = [], [], None
    for rep in range(a.reps + 2):                       # two warm-up calls
        t = {k: v.copy() for k, v in s["table"].items()}
        t0 = time.perf_counter()
        got = lcl.SearchAndFuse(table=t, **s["kw"], apply=False, cap_ops=1 << 18, cap_updated=1 << 18)
        dt = time.perf_counter() - t0
        if rep >= 2:
            walls.append(dt)
            stages.append(lcl.last_searchandfuse_timings())
    parent_route(m, s)                                  # warm-up of the old route's launches
    spent, want = parent_route(m, s)
    assert np.array_equal(got["ops"], want["ops"]) and np.array_equal(got["nfused"], want["nfused"]), "routes differ"
    st = np.median(np.stack(stages), axis=0)
    ops = got["ops"]
    kinds = np.bincount(ops[ops[:, 0] >= 0][:, 1], minlength=4)
    kinds0 = np.bincount(ops[ops[:, 0] < 0][:, 1], minlength=4)
    lines = [
        f"workload: {a.keyframes} listed keyframes, {NFEAT} features per keyframe, {NLOOP} loop points, "
        f"table {len(s['table']['bad'])} rows, {int((s['kw']['matched'] >= 0).sum())} matched entries",
        f"result: nfused sum {int(got['nfused'].sum())}, pass ops add/replace/no-op {kinds[1]}/{kinds[2]}/{kinds[3]}, "
        f"step-0 ops add/replace {kinds0[1]}/{kinds0[2]}, updated {len(got['updated'])}",
        f"LoopClosing_SearchAndFuse wall (Python call, apply=0), {a.reps} reps: median {1e3 * np.median(walls):.3f}  "
        f"min {1e3 * min(walls):.3f}  max {1e3 * max(walls):.3f} ms",
        "stages, median ms: projection %.3f  match %.3f  descriptors %.3f  host replay %.3f" % tuple(st),
        f"previous exact route, library time only (one run after a warm-up): ORBmatcher_Fuse_Sim3 x{spent['nfuse']} "
        f"{1e3 * spent['fuse']:.3f} ms + MapPoint_Update_batch x{spent['nupdate']} {1e3 * spent['update']:.3f} ms = "
        f"{1e3 * (spent['fuse'] + spent['update']):.3f} ms (the adapter's replay between the calls is not counted)",
    ]
    print("\n".join(lines))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
