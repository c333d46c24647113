#!/usr/bin/env python3
"""Time LoopClosing_CorrectLoop / LoopClosing_ApplyGlobalBA on the map shape tools/map_timing.py uses
(tests/ba_cases.global_ba_problem: 2,000 keyframes, 4 laps of one circuit, 150 points created per keyframe).

  loopcorrect_timing.py [--reps R] [--out profiles/loopcorrect_timing.txt]

Run it from the repository root.  The tables live in device memory (torch tensors, device pointers) and are
restored from a saved copy before every call, outside the clocks.  Per call two figures: the wall time of the
synchronous C call (checks, the host-side order / tree levels, launches, the downloads of the counts and the
Sim3 outputs, the wait), and the time between two HIP events recorded on the matcher's stream around it.
  * CorrectLoop: the last keyframe's covisibles (its mvpOrderedConnectedKeyFrames) and itself listed;
  * ApplyGlobalBA: the whole map from origin 0 along a parent = id - 1 spanning tree, the last 10 keyframes
    not in the BA (10 dependent steps);
  * next to them the wall time of one device -> host -> device round trip of pos, normal, max_dist and
    min_dist at that size: what a host-side correction pays before it does any arithmetic;
  * and both calls once more with host pointers (numpy tables: the staging copies are inside the call).
Absolute times only: no CPU baseline of LoopClosing.cc exists in this repository."""
import argparse
import sys
import time
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, ".")
sys.path.insert(0, str(HERE.parent / "tests"))
import numpy as np  # noqa: E402

NKF, LAPS, PPK, TAIL = 2000, 4, 150, 10


def med(ts):
    return f"median {np.median(ts):.3f}  min {min(ts):.3f}  max {max(ts):.3f} ms"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    import c_orb_slam_amd as orb
    from ba_cases import global_ba_problem
    from loopcorrect_ref import sim3_of_pose
    pr = global_ba_problem(0, n_kf=NKF, pts_per_kf=PPK, laps=LAPS)
    pe, ke = pr["edge_pt"], pr["edge_kf"]
    npt = len(pr["pt_pos"])
    order = np.argsort(ke, kind="stable")
    start = np.searchsorted(ke[order], np.arange(NKF + 1))
    rows = [pe[order[start[k]:start[k + 1]]].astype(np.int32) for k in range(NKF)]
    rng = np.random.default_rng(3)
    mp = orb.Map()
    for k, r in enumerate(rows):
        mp.AddKeyFrame(k, r)
        mp.SetKeyFrameKeys(k, rng.integers(0, 8, len(r)).astype(np.uint8))
        mp.SetNeighbours(k, [], k - 1, [k + 1] if k + 1 < NKF else [])
    cur = NKF - 1
    kf = np.append(mp.UpdateConnections(cur, cap_counter=NKF, cap_ordered=NKF)[2], cur).astype(np.int32)
    nkf_, nslot, nobs = mp.size()
    m = orb.ORBmatcher(0.8, False)
    lcl = orb.LoopClosing(m, mp)
    ref_kf = np.full(npt, -1, np.int32)
    ref_kf[pe[::-1]] = ke[::-1]                      # an observer of each point
    first_kf = np.full(npt, NKF, np.int64)
    np.minimum.at(first_kf, pe, ke)
    host = dict(Tcw=pr["kf_Tcw"].copy(), pos=pr["pt_pos"].copy(),
                normal=rng.normal(0, 1, (npt, 3)).astype(np.float32), max_dist=np.full(npt, 40, np.float32),
                min_dist=np.full(npt, 2, np.float32), ref_kf=ref_kf, corrected_ref=np.full(npt, -1, np.int32),
                bad=np.zeros(npt, np.uint8), TcwGBA=pr["kf_Tcw"].copy(),
                kf_in_gba=(np.arange(NKF) < NKF - TAIL).astype(np.uint8), posGBA=pr["pt_pos"].copy(),
                mp_in_gba=(first_kf < NKF - TAIL).astype(np.uint8), TcwBefGBA=np.zeros((NKF, 16), np.float32))
    Scw = np.array(sim3_of_pose([float(v) for v in host["Tcw"][cur]]))
    Scw[4:7] += 0.3
    Scw[7] = 1.02
    sf = np.array([1.2 ** i for i in range(8)], np.float32)
    dev = {k: torch.from_numpy(v).cuda() for k, v in host.items()}
    saved = {k: v.clone() for k, v in dev.items()}
    stream = torch.cuda.ExternalStream(orb.lib().ORBmatcher_stream(m._h))

    def correct(t):
        return lcl.CorrectLoop(kf, cur, Scw, sf, t["Tcw"], t["pos"], t["normal"], t["max_dist"], t["min_dist"],
                               t["ref_kf"], t["corrected_ref"], bad=t["bad"])

    def gba(t):
        return lcl.ApplyGlobalBA([0], t["TcwGBA"], t["kf_in_gba"], t["Tcw"], t["pos"], t["posGBA"], t["mp_in_gba"],
                                 t["ref_kf"], bad=t["bad"], TcwBefGBA=t["TcwBefGBA"])

    def timed_device(fn):
        wall, evs, out = [], [], None
        for _ in range(a.reps + 1):
            for k, v in dev.items():
                v.copy_(saved[k])
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            t0 = time.perf_counter()
            out = fn(dev)
            wall.append(1e3 * (time.perf_counter() - t0))
            e1.record(stream)
            e1.synchronize()
            evs.append(e0.elapsed_time(e1))
        return out, wall[1:], evs[1:]

    def timed_host(fn):
        wall, out = [], None
        for _ in range(a.reps + 1):
            t = {k: v.copy() for k, v in host.items()}
            t0 = time.perf_counter()
            out = fn(t)
            wall.append(1e3 * (time.perf_counter() - t0))
        return out, wall[1:]

    lines = [f"# tools/loopcorrect_timing.py --reps {a.reps}  (MI355X; medians after one warm-up call; wall = host clock "
             "around the synchronous call, events = HIP events on the matcher's stream around it)",
             f"# map: global_ba_problem(0, n_kf={NKF}, pts_per_kf={PPK}, laps={LAPS}): {nkf_} keyframes, {nslot} row slots, "
             f"{nobs} observations, {npt} map points",
             "# no CPU baseline of LoopClosing.cc exists here: absolute times only"]
    g, wall, evs = timed_device(correct)
    lines.append(f"CorrectLoop, device tables: {len(kf)} listed keyframes (the covisibles of keyframe {cur} and itself), "
                 f"{g['n_corrected']} points corrected, {g['n_ref_missing']} without their reference: wall {med(wall)} | "
                 f"events {med(evs)}")
    g, wall, evs = timed_device(gba)
    lines.append(f"ApplyGlobalBA, device tables: {NKF} keyframes reached, {g['n_kf_propagated']} propagated in {g['depth']} "
                 f"dependent steps, {g['n_mp_gba']} points from the BA, {g['n_mp_moved']} moved through their reference: "
                 f"wall {med(wall)} | events {med(evs)}")
    ts = []
    for _ in range(a.reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in ("pos", "normal", "max_dist", "min_dist"):
            dev[k].copy_(dev[k].cpu())
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    lines.append(f"round trip device -> host -> device of pos, normal, max_dist, min_dist ({npt} rows, "
                 f"{npt * 32 / 1e6:.2f} MB each way, pageable host memory): wall {med(ts[1:])}")
    g, wall = timed_host(correct)
    lines.append(f"CorrectLoop, host tables (staging inside the call): wall {med(wall)}")
    g, wall = timed_host(gba)
    lines.append(f"ApplyGlobalBA, host tables (staging inside the call): wall {med(wall)}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
