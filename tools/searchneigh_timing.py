#!/usr/bin/env python3
"""Time LocalMapping_SearchInNeighbors on a LocalMapping-sized workload: 30 target keyframes, 1,241 x 376
frames at 2,000 features, a current keyframe holding about 1,500 map points, half of the keypoints stereo.

  searchneigh_timing.py [--reps R] [--targets T] [--out profiles/searchneigh_timing.txt]

It prints
  * the stage times of the call (projection, match and descriptor recomputation summed over the passes,
    final update: HIP events; host replay: wall clock; LocalMapping_SearchInNeighbors_last_timings) and the
    call's wall time, apply = 0 so that every repetition meets the same map;
  * for the same inputs, the library time of the route an adapter had before this entry: one
    ORBmatcher_Fuse per target and one for the backward pass, one MapPoint_Update_batch between every two
    of them for the points the pass merged, and one for the final update.  Only the time inside those
    library calls is summed; the replay between them runs in Python (tests/fuse_ref.py, the same mutations)
    and is not counted, although a real adapter pays for its own.
The two routes must end with the same op log; the tool checks that before it prints.

The scene is synthetic: world points in front of the current camera, keyframes a small rotation and a few
centimetres away, keypoints = projections with 0.3 px of noise, descriptors = the point's with a few bits
flipped.  Per target and feature the keyframe holds the shared id (30 %), a duplicate point (20 %) or
nothing.  No images are extracted, so the keypoint distribution is uniform, not a KITTI one."""
import argparse
import sys
import time
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, ".")
sys.path.insert(0, str(HERE.parent / "tests"))
import numpy as np  # noqa: E402

W, H, NFEAT, NCUR = 1241, 376, 2000, 1500


def scene(ntargets, seed=0):
    import c_orb_slam_amd as orb
    from c_orb_slam_amd import synthetic
    from c_orb_slam_amd._lib import KP_DTYPE
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = synthetic.KITTI_K
    bf = synthetic.KITTI_BF
    scale = (np.float32(1.2) ** np.arange(8)).astype(np.float32)
    nw = 2600
    z = rng.uniform(8, 60, nw)
    X = np.stack([(rng.uniform(20, W - 20, nw) - cx) / fx * z, (rng.uniform(20, H - 20, nw) - cy) / fy * z, z], 1)
    base = rng.integers(0, 256, (nw, 32), dtype=np.uint8)
    octv = rng.integers(0, 6, nw)
    nkf = ntargets + 1
    cur_kf = ntargets
    T, Ow = [], np.zeros((nkf, 3), np.float32)
    for k in range(nkf):
        R = np.eye(3) if k == cur_kf else synthetic.small_rotation(rng, fx, max_shift=20.0)
        t = np.zeros(3) if k == cur_kf else rng.normal(0, 0.05, 3)
        T.append(synthetic.pose_from_rotation(R, t))
        Ow[k] = -(R.T @ t)
    pos, desc, normal, maxd, mind, ref = ([] for _ in range(6))

    def new_point(Xw, d, k, o):
        PC = Xw.astype(np.float32) - Ow[k]
        dist = np.float32(np.linalg.norm(PC))
        pos.append(Xw.astype(np.float32)); desc.append(d); normal.append(PC / dist)
        maxd.append(np.float32(dist * scale[o])); mind.append(np.float32(maxd[-1] / scale[-1])); ref.append(k)
        return len(pos) - 1

    for p in range(nw):
        new_point(X[p], base[p], cur_kf, int(octv[p]))
    frames, rows = {}, {}
    held_cur = np.zeros(nw, bool)
    for k in [cur_kf] + list(range(ntargets)):
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
        ur = np.where(rng.random(n) < 0.5, kp["x"] - bf / Xc[vis, 2], -1.0).astype(np.float32)
        frames[k] = orb.Frame(kp, d, scale, T[k], fx, fy, cx, cy, bf, W, H, uRight=ur)
        row = np.full(n, -1, np.int32)
        r = rng.random(n)
        if k == cur_kf:
            take = rng.permutation(n)[:NCUR]
            row[take] = vis[take]
            held_cur[vis[take]] = True
        else:
            for j in range(n):
                if r[j] < 0.3:
                    row[j] = vis[j]
                elif r[j] < 0.5:
                    row[j] = new_point(X[vis[j]], d[j].copy(), k, int(octv[vis[j]]))
        rows[k] = row
    ops = []
    for k in range(nkf):
        ops.append(("AddKeyFrame", k, rows[k]))
        ops.append(("SetKeyFrameKeys", k, frames[k].keysUn["octave"].astype(np.uint8), frames[k].uRight))
    n = len(pos)
    table = dict(pos=np.array(pos, np.float32).reshape(-1, 3), desc=np.array(desc, np.uint8).reshape(-1, 32),
                 normal=np.array(normal, np.float32).reshape(-1, 3), max_dist=np.array(maxd, np.float32),
                 min_dist=np.array(mind, np.float32), bad=np.zeros(n, np.uint8), ref_kf=np.array(ref, np.int32))
    kf_desc = {k: frames[k].desc for k in range(nkf)}
    tid = list(range(ntargets))
    return dict(ops=ops, table=table, frames=frames, cur_kf=cur_kf, target_ids=tid, kf_desc=kf_desc, Ow=Ow, scale=scale,
                held=int(held_cur.sum()))


def fill(target, ops):
    for op in ops:
        getattr(target, op[0])(*op[1:])
    return target


def parent_route(m, s, lsf):
    """-> (seconds inside ORBmatcher_Fuse, seconds inside MapPoint_Update_batch, calls of each, the op log)"""
    import fuse_ref
    from culling_ref import CullRefMap
    spent = dict(fuse=0.0, update=0.0, nfuse=0, nupdate=0)

    def timed_fuse(KF, pts, geo, skip, lsf_, th):
        t0 = time.perf_counter()
        out = m.Fuse(KF, pts, geo, skip, lsf_, th)
        spent["fuse"] += time.perf_counter() - t0
        spent["nfuse"] += 1
        return out

    class Route(fuse_ref.SearchInNeighborsRef):
        pending = None

        def ComputeDistinctiveDescriptors(self, p):
            if self.pending is not None and not self.isBad(p):
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

        def Fuse(self, *a):
            self.pending = {}
            n = super().Fuse(*a)
            self.flush()
            return n

    saved = fuse_ref.oracle_lib.oracle_fuse
    fuse_ref.oracle_lib.oracle_fuse = timed_fuse
    try:
        r = Route(fill(CullRefMap(), s["ops"]), s["cur_kf"], s["frames"][s["cur_kf"]], s["target_ids"],
                  [s["frames"][k] for k in s["target_ids"]], s["kf_desc"], s["Ow"], s["scale"], s["table"], lsf)
        r.pending = {}
        r.run()
        # the final update as one batch: descriptors and normal / depth of the current row's points
        fin = sorted(r.final_rows)
        if fin:
            start = np.concatenate([[0], np.cumsum([len(r.final_rows[p][1]) for p in fin])]).astype(np.int32)
            rows = np.concatenate([np.stack([s["kf_desc"][kf.mnId][idx] for kf, idx in r._observations(p)]) for p in fin])
            t0 = time.perf_counter()
            m.UpdateMapPoints(start, obs_desc=rows, pos=np.stack([r.final_rows[p][0] for p in fin]),
                              obs_Ow=np.concatenate([r.final_rows[p][1] for p in fin]),
                              ref_Ow=np.stack([r.final_rows[p][2] for p in fin]),
                              ref_scale=np.array([r.final_rows[p][3] for p in fin], np.float32),
                              ref_scale_top=np.array([r.final_rows[p][4] for p in fin], np.float32))
            spent["update"] += time.perf_counter() - t0
            spent["nupdate"] += 1
    finally:
        fuse_ref.oracle_lib.oracle_fuse = saved
    return spent, r.result()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--targets", type=int, default=30)
    ap.add_argument("--out")
    a = ap.parse_args()
    import c_orb_slam_amd as orb
    assert orb.device_available(), "searchneigh_timing.py needs a HIP device"
    s = scene(a.targets)
    lsf = np.float32(np.log(np.float32(1.2)))
    m = orb.ORBmatcher(0.6, True)
    mp = fill(orb.Map(), s["ops"])
    mp.enable_timing(True)
    cur, tg = s["frames"][s["cur_kf"]], [s["frames"][k] for k in s["target_ids"]]
    walls, stages, got = [], [], None
    for rep in range(a.reps + 2):                       # two warm-up calls
        t = {k: v.copy() for k, v in s["table"].items()}
        t0 = time.perf_counter()
        got = mp.SearchInNeighbors(m, s["cur_kf"], cur, s["target_ids"], tg, s["kf_desc"], s["Ow"], s["scale"], t, lsf,
                                   apply=False, cap_ops=1 << 17, cap_updated=1 << 17)
        dt = time.perf_counter() - t0
        if rep >= 2:
            walls.append(dt)
            stages.append(mp.last_searchneigh_timings())
    parent_route(m, s, lsf)                             # warm-up of the old route's launches
    spent, want = parent_route(m, s, lsf)
    assert np.array_equal(got["ops"], want["ops"]) and np.array_equal(got["nfused"], want["nfused"]), "routes differ"
    st = np.median(np.stack(stages), axis=0)
    kinds = np.bincount(got["ops"][:, 1], minlength=4)
    lines = [
        f"workload: {a.targets} targets, {NFEAT} features per keyframe, current row holds {s['held']} points, "
        f"table {len(s['table']['bad'])} rows",
        f"result: nfused sum {int(got['nfused'].sum())} (backward {int(got['nfused'][-1])}), ops add/replace/no-op "
        f"{kinds[1]}/{kinds[2]}/{kinds[3]}, updated {len(got['updated'])}",
        f"LocalMapping_SearchInNeighbors wall (Python call, apply=0), {a.reps} reps: median {1e3 * np.median(walls):.3f}  "
        f"min {1e3 * min(walls):.3f}  max {1e3 * max(walls):.3f} ms",
        "stages, median ms: projection %.3f  match %.3f  descriptors %.3f  final update %.3f  host replay %.3f" % tuple(st),
        f"parent route, library time only (one run after a warm-up): ORBmatcher_Fuse x{spent['nfuse']} "
        f"{1e3 * spent['fuse']:.3f} ms + MapPoint_Update_batch x{spent['nupdate']} {1e3 * spent['update']:.3f} ms = "
        f"{1e3 * (spent['fuse'] + spent['update']):.3f} ms (the adapter's replay between the calls is not counted)",
    ]
    print("\n".join(lines))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
