#!/usr/bin/env python3
"""Time the EuRoC stereo rectification (ORBextractor_remap_batch) at 752x480 with EuRoC-shaped maps,
64 stereo pairs per call (128 images, left / right interleaved through two slots), device-resident:

* the remap alone: HIP events on the extractor's stream around each call, median over the calls,
  and the achieved GB/s of its algorithmic bytes (1 B read + 1 B written per pixel and image, plus
  the 6-byte records of both slots once per call) beside the HBM peak.  The calls rotate over SETS
  source / destination buffer sets, more than the 256 MB Infinity Cache holds, so a call finds
  neither its input nor its output cached.  Measured for every setting of the images a thread makes
  from the record it holds (ORBGPU_REMAP_IPT; 1 = one image per thread, the records re-read from
  L2 by the next image's workgroups), alternating the settings call by call;
* one stereo pair per call (what a driver that does not batch enqueues per frame);
* remap -> extraction for the batch (1,200 features): HIP events from before the remap to behind
  the extraction's kernels on the same stream, and a host clock around the same calls.

  remap_timing.py [--reps R] [--out profiles/remap_timing.txt]

Run it from the repository root.  There is no CPU baseline of cv::remap in this repository, so no
speed-up is claimed.
"""
import argparse
import ctypes as C
import os
import sys
import time

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import numpy as np  # noqa: E402

W, H, PAIRS, NF, SETS = 752, 480, 64, 1200, 4
B = 2 * PAIRS
IPTS = (1, 2, 4, 8, 64)
HBM_SPEC_TBS, HBM_COPY_TBS = 8.0, 6.29   # MI355X: HBM3E spec peak; measured float4 copy


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    import c_orb_slam_amd as orb
    from c_orb_slam_amd import synthetic
    from c_orb_slam_amd._lib import check, lib, ptr
    import remap_cases as cases
    assert orb.device_available(), "no HIP device: nothing is measured without one"
    L = lib()
    dev = torch.device("cuda", 0)
    scenes, _ = synthetic.sequence(11, 4, W, H)
    raw = np.stack([cases.render_raw(scenes[(b // 2) % 4], ("left", "right")[b % 2], shift=12.0 * (b % 2))
                    for b in range(8)])
    raw = np.concatenate([raw] * (B // 8))           # left / right interleaved
    ex = orb.ORBextractor(NF, 1.2, 8, 20, 7, max_width=W, max_height=H, max_batch=B)
    for s, side in enumerate(("left", "right")):
        ex.set_remap(s, *cases.euroc_maps(side))
    es = torch.cuda.ExternalStream(ex.stream, device=dev)
    ev = lambda: torch.cuda.Event(enable_timing=True)
    lines = [f"# tools/remap_timing.py --reps {a.reps}  (MI355X; {W}x{H}, EuRoC-shaped maps, {PAIRS} stereo pairs = {B} "
             "images per call, slot_period 2; HIP events on the extractor's stream; medians over the calls after one "
             "warm-up per buffer set and setting)",
             "# no CPU baseline of cv::remap exists here: these are absolute times only, no speed-up is claimed"]

    srcs = [torch.from_numpy(raw).to(dev) for _ in range(SETS)]
    dsts = [torch.empty((B, H, W), dtype=torch.uint8, device=dev) for _ in range(SETS)]
    torch.cuda.synchronize()
    call = lambda k, n=B: ex.remap_device(srcs[k].data_ptr(), n, W, H, W, W * H, 0, 2, dsts[k].data_ptr(), W, W * H)
    pitch = 4 * ((W + 3) // 4)
    nbytes = B * W * H * 2 + 2 * pitch * H * 6

    # ---- remap alone, per images-per-thread setting (alternating, so that drift hits all alike)
    ts = {i: [] for i in IPTS}
    for i in IPTS:
        os.environ["ORBGPU_REMAP_IPT"] = str(i)
        for k in range(SETS):
            call(k)
    torch.cuda.synchronize()
    r = 0
    for _ in range(a.reps):
        for i in IPTS:
            os.environ["ORBGPU_REMAP_IPT"] = str(i)
            e0, e1 = ev(), ev()
            e0.record(es)
            call(r % SETS)
            e1.record(es)
            e1.synchronize()
            ts[i].append(e0.elapsed_time(e1))
            r += 1
    for i in IPTS:
        t = float(np.median(ts[i]))
        gbs = nbytes / (t * 1e-3) / 1e9
        lines.append(f"remap, {i:2d} image(s) per thread: median {t:.4f}  min {min(ts[i]):.4f}  max {max(ts[i]):.4f} ms per "
                     f"call = {1e3 * t / PAIRS:.2f} us per pair | {nbytes / 1e6:.1f} MB (1 B in + 1 B out per pixel, "
                     f"6 B of records per pixel and slot once) -> {gbs:.0f} GB/s = "
                     f"{100 * gbs / (1e3 * HBM_SPEC_TBS):.0f} % of the {HBM_SPEC_TBS} TB/s HBM3E spec peak, "
                     f"{100 * gbs / (1e3 * HBM_COPY_TBS):.0f} % of the {HBM_COPY_TBS} TB/s a float4 copy reaches | "
                     f"{SETS} buffer sets in rotation ({SETS * 2 * B * W * H / 1e6:.0f} MB > 256 MB Infinity Cache)")
    del os.environ["ORBGPU_REMAP_IPT"]           # the library's default from here on

    # ---- one pair per call
    tp = []
    for k in range(SETS):
        call(k, 2)
    torch.cuda.synchronize()
    for r in range(a.reps):
        e0, e1 = ev(), ev()
        e0.record(es)
        call(r % SETS, 2)
        e1.record(es)
        e1.synchronize()
        tp.append(e0.elapsed_time(e1))
    lines.append(f"remap, one pair per call (library default): median {1e3 * float(np.median(tp)):.1f}  "
                 f"min {1e3 * min(tp):.1f}  max {1e3 * max(tp):.1f} us (events around one launch: mostly launch latency)")

    # ---- remap -> extraction
    cap = 2 * NF + 64
    d_k = torch.zeros((B, cap, 7), dtype=torch.int32, device=dev)
    d_d = torch.zeros((B, cap, 32), dtype=torch.uint8, device=dev)
    n = np.zeros(B, np.int32)

    def chain(k):
        call(k)
        check(L.ORBextractor_extract_batch(ex._h, C.c_void_p(dsts[k].data_ptr()), B, W, H, W, W * H, 1,
                                           C.c_void_p(d_k.data_ptr()), C.c_void_p(d_d.data_ptr()), cap, 1, ptr(n)))

    def extract_only(k):
        check(L.ORBextractor_extract_batch(ex._h, C.c_void_p(dsts[k].data_ptr()), B, W, H, W, W * H, 1,
                                           C.c_void_p(d_k.data_ptr()), C.c_void_p(d_d.data_ptr()), cap, 1, ptr(n)))

    for k in range(SETS):
        chain(k)
    torch.cuda.synchronize()
    te, th, tx = [], [], []
    for r in range(a.reps):
        for fn, evs, hs in ((chain, te, th), (extract_only, tx, None)):
            e0, e1 = ev(), ev()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record(es)
            fn(r % SETS)                             # extract_batch returns after its counts have arrived
            dt = time.perf_counter() - t0
            e1.record(es)
            e1.synchronize()
            evs.append(e0.elapsed_time(e1))
            if hs is not None:
                hs.append(dt)
    t, hm, x = float(np.median(te)), 1e3 * float(np.median(th)), float(np.median(tx))
    lines.append(f"remap -> extraction ({B} images per call, {NF} features, mean {n.mean():.0f} keypoints): HIP events "
                 f"median {t:.3f}  min {min(te):.3f}  max {max(te):.3f} ms = {PAIRS / (t * 1e-3):.0f} stereo pairs/s | host "
                 f"clock median {hm:.3f} ms | extraction alone on the rectified images: median {x:.3f} ms, so the remap "
                 f"adds {t - x:.3f} ms per call = {1e3 * (t - x) / PAIRS:.2f} us per pair")
    lines.append("# not measured: host-resident raw images (the H2D copy), cv::initUndistortRectifyMap (the driver's, once "
                 "per camera), and a remap fused into the pyramid's level 0 (not built)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
