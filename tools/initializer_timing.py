#!/usr/bin/env python3
"""Time Initializer_Initialize at N = 100, 500 and 2,000 matches with 200 iterations: ms per call
by a host clock around the synchronous C call (arguments built once, outside the clock), and the
four kernels by HIP events on the handle's stream (Initializer_enable_timing), after a warm-up.
The event pass is a second set of calls, so the host-clock numbers carry no event overhead.

  initializer_timing.py [--reps R] [--out profiles/initializer_timing.txt]

Run it from the repository root: the scenes come from tests/initializer_cases.py.  There is no
CPU baseline of Initializer.cc on this machine, so no speed-up is claimed.
"""
import argparse
import ctypes as C
import sys
import time

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out")
    a = ap.parse_args()
    import initializer_cases as ic
    from c_orb_slam_amd._lib import lib, ptr
    from c_orb_slam_amd.ransac import Initializer, Rng
    L = lib()
    lines = [f"# tools/initializer_timing.py --reps {a.reps}  (MI355X; 200 iterations; host clock around the synchronous "
             "C call; kernels by HIP events in a second pass; medians over the calls after one warm-up)",
             "# no CPU baseline of Initializer.cc exists here: these are absolute times only"]
    for N in (100, 500, 2000):
        s = ic.scene("general", 1, N, 0.1)
        I = Initializer(s["K"], s["keys1"], 1.0, 200)
        n1, n2 = len(s["keys1"]), len(s["keys2"])
        R, t = np.zeros(9, np.float32), np.zeros(3, np.float32)
        P, tri = np.zeros((n1, 3), np.float32), np.zeros(n1, np.uint8)
        ok = C.c_int()

        def call():
            g = Rng(0)
            rc = L.Initializer_Initialize(I._h, n2, ptr(s["keys2"]), ptr(s["matches12"]), C.byref(g.s), ptr(R), ptr(t),
                                          ptr(P), ptr(tri), C.byref(ok), None)
            assert rc == 0, rc

        call()                                # warm-up: buffer growth, code object load
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            call()
            ts.append(time.perf_counter() - t0)
        I.enable_timing(True)
        call()
        ks = []
        for _ in range(a.reps):
            call()
            ks.append(I.last_timings().copy())
        I.close()
        k = 1e3 * np.median(np.array(ks), axis=0)
        lines.append(f"N {N:5d} (n1 {n1}, n2 {n2}, ok {ok.value}): call median {1e3 * np.median(ts):.3f}  "
                     f"min {1e3 * min(ts):.3f}  max {1e3 * max(ts):.3f} ms | kernels (us) hypotheses {k[0]:.1f}  "
                     f"select {k[1]:.1f}  check_rt {k[2]:.1f}  finish {k[3]:.1f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
