"""One ORB extraction run in a fresh process (tests/test_gpu_extract_paths.py), for the opt-in paths
whose environment variables the library reads once per process (ORBGPU_PYR_CHAIN,
ORBGPU_PYR_CHAIN_FROM, ORBGPU_BLUR_EARLY): two different batches of B images through one extractor;
every image's keypoints, descriptors, padded levels and blurred levels, and the plan flags of each
call (orbgpu_debug_extract_plan), go to <out>.  The parent sets the variables and compares with the
oracle.
usage: extract_path_worker.py <W> <H> <scaleFactor> <nlevels> <nfeatures> <B> <out.npz>"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

CALLS = 2


def batch_images(W, H, B, call):
    import extract_cases as ec
    return np.stack([ec.image(W, H, 1 + call * B + b) for b in range(B)])


def main():
    W, H, sf, nl, nf, B, out = sys.argv[1:8]
    W, H, sf, nl, nf, B = int(W), int(H), float(sf), int(nl), int(nf), int(B)
    import c_orb_slam_amd as orb
    import extract_cases as ec
    ex = orb.ORBextractor(nf, sf, nl, 20, 7, max_width=W, max_height=H, max_batch=B)
    res = {}
    for call in range(CALLS):
        kd = ex.extract_batch(batch_images(W, H, B, call))
        flags, chain_from, rows = ec.extract_plan(ex)
        res[f"c{call}_plan"] = np.array([flags, chain_from], np.int32)
        res[f"c{call}_tile_rows"] = rows
        for b in range(B):
            res[f"c{call}_b{b}_kps"] = kd[b][0]
            res[f"c{call}_b{b}_desc"] = kd[b][1]
            for l in range(nl):
                res[f"c{call}_b{b}_level{l}"] = ex.image_pyramid_level(l, b)
                res[f"c{call}_b{b}_blur{l}"] = ex.blurred_level(l, b)
    np.savez(out, **res)
    print(f"{W}x{H} x{sf} {nl} levels, B {B}: plans {[res[f'c{c}_plan'].tolist() for c in range(CALLS)]}", flush=True)


if __name__ == "__main__":
    main()
