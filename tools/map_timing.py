#!/usr/bin/env python3
"""Time the Map handle on the map shape the global-BA bench uses (tests/ba_cases.global_ba_problem:
2,000 keyframes, 4 laps of one circuit, 150 points created per keyframe) with a batch of 64 frames.

  map_timing.py [--reps R] [--out profiles/map_timing.txt] [--dump lists.npz]
  map_timing.py --host-table lists.npz [--reps R] [--append profiles/map_timing.txt]

The first form needs this commit's library.  It records
  * the HIP-event times of Tracking_UpdateLocalMap_batch's stages (index rebuild, vote, keyframe
    selection, local points, remap + gather; Map_last_timings) for the batch in one chunk;
  * the host time of one deferred TrackLocalMap chain of the 64 frames with the new call in it:
    Tracking_UpdateLocalMap_batch -> Tracking_PrepareLocalSearch_batch_device ->
    ORBmatcher_SearchLocalPoints_batch -> ORBmatcher_finish (first call to the return of finish);
  * the same chain without the new call, fed the local maps built on the host beforehand from the
    same lists (outside the clock), which is what a tracker had to do before;
and with --dump writes the lists for the second form.  The second form runs that host-table chain
only and uses nothing this commit adds, so it can be run from a checkout of the parent commit
(python <this file> from that checkout's root) to put the parent's figure next to the others.

Frame f is keyframe k_f of the map seen again: its keypoints are that keyframe's observations, 15 % of
them already hold their map point (what TrackWithMotionModel leaves), descriptors are the points' with one
bit flipped.  The local map of such a frame is far larger than a KITTI one (every keyframe of the map sees
~1,000 points and the circuit is driven four times), so the figures are an upper range, and they are
absolute times: no CPU baseline of Tracking::UpdateLocalMap exists in this repository.
"""
import argparse
import ctypes as C
import sys
import time
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, ".")
sys.path.insert(0, str(HERE.parent / "tests"))
import numpy as np  # noqa: E402

NKF, LAPS, PPK, BATCH, KF_CAP = 2000, 4, 150, 64, 128
W, H = 1241, 376


def scene():
    from ba_cases import KITTI, global_ba_problem
    pr = global_ba_problem(0, n_kf=NKF, pts_per_kf=PPK, laps=LAPS)
    pe, ke, ob = pr["edge_pt"], pr["edge_kf"], pr["edge_obs"]
    npt = len(pr["pt_pos"])
    rng = np.random.default_rng(1)
    order = np.argsort(ke, kind="stable")
    start = np.searchsorted(ke[order], np.arange(NKF + 1))
    rows = [pe[order[start[k]:start[k + 1]]].astype(np.int32) for k in range(NKF)]
    Tcw = pr["Tcw_true"]
    Ow = np.stack([-T[:3, :3].T @ T[:3, 3] for T in Tcw])
    # the table: the MapPoint fields isInFrustum / SearchByProjection read, from the first observer
    _, first = np.unique(pe, return_index=True)
    X = pr["Xw_true"]
    v = X - Ow[ke[first]]
    d = np.linalg.norm(v, axis=1)
    scale = (np.float32(1.2) ** np.arange(8)).astype(np.float32)
    table = dict(pos=X.astype(np.float32), desc=rng.integers(0, 256, (npt, 32), dtype=np.uint8),
                 obs=np.bincount(pe, minlength=npt).astype(np.int32), max_dist=(d * 1.2 ** 3).astype(np.float32),
                 min_dist=(d * 1.2 ** 3 / scale[7]).astype(np.float32), normal=(v / d[:, None]).astype(np.float32),
                 skip=np.zeros(npt, np.uint8))
    import c_orb_slam_amd as orb
    from c_orb_slam_amd._lib import KP_DTYPE
    fx, fy, cx, cy, bf = (float(x) for x in KITTI)
    frames, cur = [], []
    for k in rng.choice(NKF, BATCH, replace=False):
        e = order[start[k]:start[k + 1]]
        kp = np.zeros(len(e), KP_DTYPE)
        kp["x"], kp["y"] = np.clip(ob[e, 0], 1, W - 2), np.clip(ob[e, 1], 1, H - 2)
        kp["octave"] = rng.integers(0, 8, len(e))
        kp["size"] = 31
        dsc = table["desc"][pe[e]].copy()
        dsc[np.arange(len(e)), rng.integers(0, 32, len(e))] ^= np.uint8(1) << rng.integers(0, 8, len(e)).astype(np.uint8)
        frames.append(orb.Frame(kp, dsc, scale, Tcw[k].astype(np.float32), fx, fy, cx, cy, bf, W, H,
                                uRight=ob[e, 2].astype(np.float32)))
        cur.append(np.where(rng.random(len(e)) < 0.15, pe[e], -1).astype(np.int32))
    return rows, table, frames, cur, scale


def med(ts):
    return f"median {1e3 * np.median(ts):.3f}  min {1e3 * min(ts):.3f}  max {1e3 * max(ts):.3f} ms"


def host_table_chain(m, frames, table, lists, reps):
    """PrepareLocalSearch -> SearchLocalPoints -> finish, deferred, over local maps gathered on the host."""
    import torch
    from c_orb_slam_amd._lib import lib, orb_localmap, orb_localprep, ptr
    L = lib()
    dev = torch.device("cuda", 0)
    maps = []
    for lp in lists["local_mp"]:
        maps.append({k: np.asarray(table[k])[lp] for k in ("pos", "desc", "obs", "max_dist", "min_dist", "normal")})
        maps[-1]["skip"] = np.zeros(len(lp), np.uint8)
    keep, fa, ma = m._local_batch(frames, maps, dev)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    crow0 = [t(c) for c in lists["cur_row"]]
    crow = [c.clone() for c in crow0]
    outl = [torch.zeros(len(c), dtype=torch.uint8, device=dev) for c in crow0]
    rowt = [torch.arange(len(lp), dtype=torch.int32, device=dev) for lp in lists["local_mp"]]
    n = len(frames)
    prep = (orb_localprep * n)(*[orb_localprep(F.N, c.data_ptr(), o.data_ptr(), len(lp), r.data_ptr(), k["skip"].data_ptr())
                                 for F, c, o, lp, r, k in zip(frames, crow, outl, lists["local_mp"], rowt, keep)])
    cm = (C.c_void_p * n)(*[c.data_ptr() for c in crow])
    nm, nv = np.zeros(n, np.int32), np.zeros(n, np.int32)
    lsf = float(np.float32(np.log(np.float32(1.2))))
    assert L.ORBmatcher_set_device_pointers(m._h, 1) == 0 and L.ORBmatcher_set_deferred(m._h, 1) == 0
    ts = []
    for r in range(reps + 1):
        for c, c0 in zip(crow, crow0):
            c.copy_(c0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        assert L.Tracking_PrepareLocalSearch_batch_device(m._h, n, prep) == 0
        assert L.ORBmatcher_SearchLocalPoints_batch(m._h, n, fa, cm, ma, lsf, 1.0, 0.8, ptr(nm), ptr(nv)) == 0
        assert L.ORBmatcher_finish(m._h) == 0
        ts.append(time.perf_counter() - t0)
    assert L.ORBmatcher_set_deferred(m._h, 0) == 0 and L.ORBmatcher_set_device_pointers(m._h, 0) == 0
    del keep
    return ts[1:], int(nm.sum()), int(nv.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out")
    ap.add_argument("--dump")
    ap.add_argument("--host-table")
    ap.add_argument("--append")
    a = ap.parse_args()
    import torch  # noqa: F401  (its HIP runtime first, as the tests and the bench load it)
    import c_orb_slam_amd as orb
    rows, table, frames, cur, scale = scene()
    if a.host_table:
        z = np.load(a.host_table)
        lists = dict(local_mp=[z[f"lp{f}"] for f in range(BATCH)], cur_row=[z[f"cr{f}"] for f in range(BATCH)])
        ts, nm, nv = host_table_chain(orb.ORBmatcher(0.8, False), frames, table, lists, a.reps)
        line = (f"chain without the call, host-built local maps, library of the checkout at {Path('.').resolve().name}: "
                f"{med(ts)}  (matches {nm}, visible {nv})\n")
        print(line, end="")
        if a.append:
            open(a.append, "a").write(line)
        return
    import torch
    from c_orb_slam_amd._lib import lib, orb_localmap, orb_localprep, orb_localupdate, ptr
    L = lib()
    dev = torch.device("cuda", 0)
    npt = len(table["pos"])
    assert L.orbgpu_unit_set_map_chunk(BATCH) == 0
    mp = orb.Map()
    t0 = time.perf_counter()
    for k, r in enumerate(rows):
        mp.AddKeyFrame(k, r)
    t_add = time.perf_counter() - t0
    t0 = time.perf_counter()
    conn = mp.UpdateConnections_batch(np.arange(NKF), cap_counter=NKF, cap_ordered=NKF)
    t_conn = time.perf_counter() - t0
    children = [[] for _ in range(NKF)]
    parent = np.full(NKF, -1)
    for k in range(1, NKF):   # the first connection of an earlier id, as UpdateConnections picks it at creation
        older = [int(i) for i in conn[k][2] if i < k]
        if older:
            parent[k] = older[0]
            children[older[0]].append(k)
    for k in range(NKF):
        mp.SetNeighbours(k, conn[k][2][:10], int(parent[k]), children[k])
    m = orb.ORBmatcher(0.8, False)
    nkf_, nslot, nobs = mp.size()
    lines = [f"# tools/map_timing.py --reps {a.reps}  (MI355X; medians after one warm-up call)",
             f"# map: global_ba_problem(0, n_kf={NKF}, pts_per_kf={PPK}, laps={LAPS}): {nkf_} keyframes, {nslot} row slots, "
             f"{nobs} observations, {npt} map points; batch of {BATCH} frames, each a keyframe of the map seen again",
             "# no CPU baseline of Tracking::UpdateLocalMap / KeyFrame::UpdateConnections exists here: absolute times only",
             f"build: {NKF} Map_AddKeyFrame calls {1e3 * t_add:.1f} ms (host mirror); KeyFrame_UpdateConnections_batch of "
             f"all {NKF} keyframes {1e3 * t_conn:.1f} ms (first query: upload + index build included)"]
    # ---- stages (host pointers, one chunk)
    res = m.UpdateLocalMap(mp, [c.copy() for c in cur], bad=table["skip"], kf_cap=KF_CAP, pt_cap=1 << 16)
    n_kf = np.array([r["n_kf"] for r in res])
    n_pt = np.array([r["n_pt"] for r in res])
    pt_cap = int((n_pt.max() + 1023) // 1024 * 1024)
    lines.append(f"per frame: keypoints {np.mean([F.N for F in frames]):.0f}, with a point {np.mean([(c >= 0).sum() for c in cur]):.0f}; "
                 f"local keyframes mean {n_kf.mean():.1f} max {n_kf.max()}; local points mean {n_pt.mean():.0f} max {n_pt.max()}")
    mp.enable_timing(True)
    ks, rb, calls = [], [], []
    for r in range(a.reps + 1):
        if r % 2 == 0:   # every other call follows a mutation: one slot of one row, then the index is rebuilt
            mp.SetMapPointMatches(int(r), [0], [int(rows[r][0])], [r % 4 == 0])
        t0 = time.perf_counter()
        m.UpdateLocalMap(mp, [c.copy() for c in cur], bad=table["skip"], kf_cap=KF_CAP, pt_cap=pt_cap)
        calls.append(time.perf_counter() - t0)
        k = mp.last_timings()
        ks.append(k[1:].copy())
        if k[0] >= 0:
            rb.append(k[0])
    k = np.median(np.array(ks[1:]), axis=0)
    lines.append(f"Tracking_UpdateLocalMap_batch x{BATCH}, host pointers (lists only), HIP events (ms): index rebuild "
                 f"{np.median(rb[1:]):.3f} (upload of the changed row + count, scan, fill over {nobs} observations) | "
                 f"vote {k[0]:.3f}  keyframe selection {k[1]:.3f}  local points {k[2]:.3f}  remap {k[3]:.3f}")
    lines.append(f"  the synchronous host-pointer call (staging and downloads included): {med(calls[1:])}")
    mp.enable_timing(False)
    # ---- the deferred chain with the call in it (device pointers, gather)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    T = {k: t(table[k]) for k in ("pos", "desc", "obs", "max_dist", "min_dist", "normal", "skip")}
    tab = orb_localmap(npt, T["pos"].data_ptr(), T["desc"].data_ptr(), T["obs"].data_ptr(), T["max_dist"].data_ptr(),
                       T["min_dist"].data_ptr(), T["normal"].data_ptr(), T["skip"].data_ptr())
    dummy = dict(pos=np.zeros((1, 3), np.float32), max_dist=np.zeros(1, np.float32), min_dist=np.zeros(1, np.float32),
                 normal=np.zeros((1, 3), np.float32), skip=np.zeros(1, np.uint8))
    keep, fa, _ = m._local_batch(frames, [dummy] * BATCH, dev)
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
    ua = (orb_localupdate * BATCH)()
    O, cur0 = [], [t(c) for c in cur]
    for u, c in zip(ua, cur):
        o = dict(cur=t(c), kf=z((KF_CAP,), torch.int32), lp=z((pt_cap,), torch.int32), crow=z((len(c),), torch.int32),
                 row=z((pt_cap,), torch.int32), pos=z((pt_cap, 3), torch.float32), desc=z((pt_cap, 32), torch.uint8),
                 obs=z((pt_cap,), torch.int32), mx=z((pt_cap,), torch.float32), mn=z((pt_cap,), torch.float32),
                 nrm=z((pt_cap, 3), torch.float32), skip=z((pt_cap,), torch.uint8), outl=z((len(c),), torch.uint8))
        u.N, u.cur_mp, u.table, u.kf_cap, u.pt_cap = len(c), o["cur"].data_ptr(), C.pointer(tab), KF_CAP, pt_cap
        u.local_kf, u.local_mp, u.cur_row, u.row = (o[k].data_ptr() for k in ("kf", "lp", "crow", "row"))
        u.pos, u.desc, u.observations, u.max_dist, u.min_dist, u.normal, u.skip = (
            o[k].data_ptr() for k in ("pos", "desc", "obs", "mx", "mn", "nrm", "skip"))
        O.append(o)
    prep = (orb_localprep * BATCH)(*[orb_localprep(len(c), o["crow"].data_ptr(), o["outl"].data_ptr(), pt_cap,
                                                   o["row"].data_ptr(), o["skip"].data_ptr()) for c, o in zip(cur, O)])
    maps = (orb_localmap * BATCH)(*[orb_localmap(pt_cap, o["pos"].data_ptr(), o["desc"].data_ptr(), o["obs"].data_ptr(),
                                                 o["mx"].data_ptr(), o["mn"].data_ptr(), o["nrm"].data_ptr(),
                                                 o["skip"].data_ptr()) for o in O])
    cm = (C.c_void_p * BATCH)(*[o["crow"].data_ptr() for o in O])
    nm, nv = np.zeros(BATCH, np.int32), np.zeros(BATCH, np.int32)
    lsf = float(np.float32(np.log(np.float32(1.2))))
    assert L.ORBmatcher_set_device_pointers(m._h, 1) == 0 and L.ORBmatcher_set_deferred(m._h, 1) == 0
    ts, tu = [], []
    for r in range(a.reps + 1):
        for o, c0 in zip(O, cur0):
            o["cur"].copy_(c0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        assert L.Tracking_UpdateLocalMap_batch(m._h, mp._h, BATCH, ua) == 0
        t1 = time.perf_counter()
        assert L.Tracking_PrepareLocalSearch_batch_device(m._h, BATCH, prep) == 0
        assert L.ORBmatcher_SearchLocalPoints_batch(m._h, BATCH, fa, cm, maps, lsf, 1.0, 0.8, ptr(nm), ptr(nv)) == 0
        assert L.ORBmatcher_finish(m._h) == 0
        ts.append(time.perf_counter() - t0)
        tu.append(t1 - t0)
    assert L.ORBmatcher_set_deferred(m._h, 0) == 0 and L.ORBmatcher_set_device_pointers(m._h, 0) == 0
    assert [u.n_pt for u in ua] == n_pt.tolist() and [u.n_kf for u in ua] == n_kf.tolist()
    # the stages of the device-pointer call, whose last stage gathers the table's rows (synchronous calls)
    mp.enable_timing(True)
    assert L.ORBmatcher_set_device_pointers(m._h, 1) == 0
    kd = []
    for r in range(a.reps + 1):
        for o, c0 in zip(O, cur0):
            o["cur"].copy_(c0)
        torch.cuda.synchronize()
        assert L.Tracking_UpdateLocalMap_batch(m._h, mp._h, BATCH, ua) == 0
        kd.append(mp.last_timings()[1:].copy())
    assert L.ORBmatcher_set_device_pointers(m._h, 0) == 0
    mp.enable_timing(False)
    k = np.median(np.array(kd[1:]), axis=0)
    gb = float(n_pt.sum()) * (12 + 32 + 4 + 4 + 4 + 12) * 2 / 1e6
    lines.append(f"Tracking_UpdateLocalMap_batch x{BATCH}, device pointers, HIP events (ms): vote {k[0]:.3f}  keyframe "
                 f"selection {k[1]:.3f}  local points {k[2]:.3f}  remap + gather {k[3]:.3f} ({int(n_pt.sum())} rows of "
                 f"68 B read and written: {gb:.1f} MB, plus the padding's row / skip)")
    lines.append(f"deferred chain x{BATCH}, UpdateLocalMap -> PrepareLocalSearch -> SearchLocalPoints -> finish "
                 f"(local maps of pt_cap = {pt_cap} rows, padding skipped): {med(ts[1:])}  (matches {int(nm.sum())}, "
                 f"visible {int(nv.sum())}); host time inside the new call {1e3 * np.median(tu[1:]):.3f} ms")
    lists = dict(local_mp=[r["local_mp"] for r in res], cur_row=[r["cur_row"] for r in res])
    ts2, nm2, nv2 = host_table_chain(m, frames, table, lists, a.reps)
    lines.append(f"chain without the call, host-built local maps of n_pt rows, this commit's library: {med(ts2)}  "
                 f"(matches {nm2}, visible {nv2})")
    if a.dump:
        np.savez(a.dump, **{f"lp{f}": r["local_mp"] for f, r in enumerate(res)},
                 **{f"cr{f}": r["cur_row"] for f, r in enumerate(res)})
    del keep
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
