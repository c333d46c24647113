#!/usr/bin/env python3
"""Time the RGB-D frame input at 640x480, 1,000 features, batch 64, everything device-resident:

* the grey conversion (ORBextractor_cvtColor_batch, 3 and 4 channels): HIP events on the
  extractor's stream around each call, median over the calls, and the achieved GB/s of its
  algorithmic bytes (channels + 1 per pixel) beside the HBM peak.  The calls rotate over SETS
  source / destination buffer sets, more than the 256 MB Infinity Cache holds, so a call finds
  neither its input nor its output cached;
* the depth gather (Frame_ComputeStereoFromRGBD_batch, U16 depth, device pointers): HIP events on
  the matcher's stream around the call (count memset, launches, count readback);
* the whole RGB-D frame construction -- cvtColor -> extraction -> UndistortKeyPoints ->
  ComputeStereoFromRGBD -- as frames/s: HIP events from the extractor's stream before the grey
  conversion to the matcher's stream behind the depth gather, and a host clock around the same
  calls (the last one ends in a stream synchronise).  The C structs are built once, outside the
  clock.

  rgbd_timing.py [--reps R] [--out profiles/rgbd_timing.txt]

Run it from the repository root.  There is no CPU baseline of these steps (cv::cvtColor,
cv::Mat::convertTo, Frame::ComputeStereoFromRGBD) in this repository, so no speed-up is claimed.
"""
import argparse
import ctypes as C
import sys
import time

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import numpy as np  # noqa: E402

W, H, B, NF, SETS = 640, 480, 64, 1000, 6
HBM_SPEC_TBS, HBM_COPY_TBS = 8.0, 6.29   # MI355X: HBM3E spec peak; measured float4 copy


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    import c_orb_slam_amd as orb
    from c_orb_slam_amd import synthetic
    from c_orb_slam_amd._lib import check, lib, orb_rgbd, orb_undistort, ptr
    import rgbd_cases as cases
    from undistort_cases import CAMERAS, K_of
    assert orb.device_available(), "no HIP device: nothing is measured without one"
    L = lib()
    dev = torch.device("cuda", 0)
    cam, dist, _, _ = CAMERAS["tum1"]
    rng = np.random.default_rng(1)
    grays, _ = synthetic.sequence(11, 8, W, H)
    color3 = np.stack([cases.spread_gray(rng, grays[b % 8]) for b in range(B)])
    color4 = np.concatenate([color3, rng.integers(0, 256, (B, H, W, 1), dtype=np.uint8)], axis=3)
    ex = orb.ORBextractor(NF, 1.2, 8, 20, 7, max_width=W, max_height=H, max_batch=B)
    m = orb.ORBmatcher(0.9, True)
    es = torch.cuda.ExternalStream(ex.stream, device=dev)
    ms = torch.cuda.ExternalStream(L.ORBmatcher_stream(m._h), device=dev)
    ev = lambda: torch.cuda.Event(enable_timing=True)
    lines = [f"# tools/rgbd_timing.py --reps {a.reps}  (MI355X; {W}x{H}, {NF} features, batch {B}; HIP events on the "
             "library's streams; medians over the calls after one warm-up per buffer set)",
             "# no CPU baseline of cv::cvtColor / convertTo / Frame::ComputeStereoFromRGBD exists here: these are "
             "absolute times only, no speed-up is claimed"]

    # ---- grey conversion
    d_gray = [torch.empty((B, H, W), dtype=torch.uint8, device=dev) for _ in range(SETS)]
    for ch, col in ((3, color3), (4, color4)):
        srcs = [torch.from_numpy(col).to(dev) for _ in range(SETS)]
        torch.cuda.synchronize()
        call = lambda k: ex.cvtColor_device(srcs[k].data_ptr(), B, W, H, ch, True, ch * W, ch * W * H,
                                            d_gray[k].data_ptr(), W, W * H)
        for k in range(SETS):
            call(k)
        torch.cuda.synchronize()
        ts = []
        for r in range(a.reps):
            e0, e1 = ev(), ev()
            e0.record(es)
            call(r % SETS)
            e1.record(es)
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        nbytes = B * W * H * (ch + 1)
        t = float(np.median(ts))
        gbs = nbytes / (t * 1e-3) / 1e9
        lines.append(f"cvtColor {ch} ch: median {t:.4f}  min {min(ts):.4f}  max {max(ts):.4f} ms per call | "
                     f"{nbytes / 1e6:.1f} MB ({ch} B in + 1 B out per pixel) -> {gbs:.0f} GB/s = "
                     f"{100 * gbs / (1e3 * HBM_SPEC_TBS):.0f} % of the {HBM_SPEC_TBS} TB/s HBM3E spec peak, "
                     f"{100 * gbs / (1e3 * HBM_COPY_TBS):.0f} % of the {HBM_COPY_TBS} TB/s a float4 copy reaches | "
                     f"{SETS} buffer sets in rotation ({SETS * nbytes / 1e6:.0f} MB > 256 MB Infinity Cache)")
        del srcs

    # ---- buffers of the frame chain
    cap = 2 * NF + 64
    d_col = torch.from_numpy(color3).to(dev)
    d_k = torch.zeros((B, cap, 7), dtype=torch.int32, device=dev)
    d_d = torch.zeros((B, cap, 32), dtype=torch.uint8, device=dev)
    d_u = torch.zeros_like(d_k)
    depth = cases.depth_u16(rng, H, W)
    d_depth = torch.from_numpy(depth).to(dev)
    d_uR = torch.zeros((B, cap), device=dev)
    d_z = torch.zeros((B, cap), device=dev)
    torch.cuda.synchronize()
    n = np.zeros(B, np.int32)
    nd = np.zeros(B, np.int32)

    def grey_extract():
        ex.cvtColor_device(d_col.data_ptr(), B, W, H, 3, True, 3 * W, 3 * W * H, d_gray[0].data_ptr(), W, W * H)
        check(L.ORBextractor_extract_batch(ex._h, C.c_void_p(d_gray[0].data_ptr()), B, W, H, W, W * H, 1,
                                           C.c_void_p(d_k.data_ptr()), C.c_void_p(d_d.data_ptr()), cap, 1, ptr(n)))

    grey_extract()   # warm-up; the counts are those of every later call (same images)
    us = (orb_undistort * B)(*[m._undistort_struct(int(n[b]), d_k[b].data_ptr(), d_u[b].data_ptr(),
                                                                K_of(cam), np.float32(dist)) for b in range(B)])
    rs = (orb_rgbd * B)(*[orb_rgbd(int(n[b]), d_k[b].data_ptr(), d_u[b].data_ptr(), d_depth.data_ptr(), 0, W, H,
                                   2 * W, float(cases.TUM_FACTOR), 40.0, d_uR[b].data_ptr(), d_z[b].data_ptr())
                          for b in range(B)])
    check(L.ORBmatcher_set_device_pointers(m._h, 1))

    def frame_tail():
        check(L.Frame_UndistortKeyPoints_batch(m._h, B, us))
        check(L.Frame_ComputeStereoFromRGBD_batch(m._h, B, rs, ptr(nd)))   # ends in the matcher's stream sync

    frame_tail()
    torch.cuda.synchronize()

    # ---- depth gather alone
    ts = []
    for _ in range(a.reps):
        e0, e1 = ev(), ev()
        e0.record(ms)
        check(L.Frame_ComputeStereoFromRGBD_batch(m._h, B, rs, ptr(nd)))
        e1.record(ms)
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    t = float(np.median(ts))
    lines.append(f"depth gather ({B} frames, {int(n.sum())} keypoints, {int(nd.sum())} with depth; U16 {W}x{H}, factor "
                 f"1/5000): median {t:.4f}  min {min(ts):.4f}  max {max(ts):.4f} ms per call "
                 f"(count memset + {(B + 43) // 44} launches + count readback) = {1e3 * t / B:.2f} us per frame")

    # ---- the whole frame construction
    te, th = [], []
    for _ in range(a.reps):
        e0, e1 = ev(), ev()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record(es)
        grey_extract()
        frame_tail()
        th.append(time.perf_counter() - t0)
        e1.record(ms)
        e1.synchronize()
        te.append(e0.elapsed_time(e1))
    t, hm = float(np.median(te)), 1e3 * float(np.median(th))
    lines.append(f"RGB-D frame construction (cvtColor 3 ch + extraction + UndistortKeyPoints + ComputeStereoFromRGBD, "
                 f"{B} frames per call, mean {n.mean():.0f} keypoints): HIP events median {t:.3f}  min {min(te):.3f}  "
                 f"max {max(te):.3f} ms = {B / (t * 1e-3):.0f} frames/s | host clock median {hm:.3f} ms = "
                 f"{B / (hm * 1e-3):.0f} frames/s")
    lines.append("# not measured: host-resident colour or depth input (the H2D copies), 16-bit PNG decoding, and the "
                 "grey conversion fused into the pyramid's level 0 (not built)")
    check(L.ORBmatcher_set_device_pointers(m._h, 0))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
