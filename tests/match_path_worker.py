"""The guided matcher's fixed case list in a fresh process (tests/test_gpu_match_paths.py), for the
instantiations chosen by environment variables the library reads once per process
(ORBGPU_CAND_NT, ORBGPU_SELECT_LOCAL_NT, ORBGPU_CAND_LOCAL_STAGE): every case's counts, cur_mp
arrays and launch plan (ORBmatcher_last_search_plan) go to <out>.  The parent sets the variables
and compares with the oracle.
usage: match_path_worker.py <out.npz>"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

LAST_CASES = ("mix-300", "mix-1536a")                 # SearchByProjection(Cur, Last), th 15
LOCAL_CASES = (("mix-300", 200), ("mix-300", 4700))   # SearchByProjection(F, map points), th 5
BATCH_NP = 9                                          # SearchLocalPoints, th 3
PLAN_KEYS = ("staged", "cand_threads", "select_threads", "max_n", "max_q", "np")


def local_queries(cid, nq):
    """The queries past k_select_r's 4,096 slots are drawn from half of the map points, held out of
    the earlier queries: a 300-keypoint frame leaves late queries few free keypoints otherwise."""
    import match_cases as mc
    return mc.local_of(cid, nq, max(nq - mc.SLOT_QUERIES, 0), 0.5)


def main():
    out = sys.argv[1]
    # torch (SearchLocalPoints' device tensors) bundles its own HIP runtime under the same soname as
    # the system's: load it before liborbslam_gpu.so so that both use one copy, as tests/conftest.py does
    import torch  # noqa: F401
    import c_orb_slam_amd as orb
    import match_cases as mc
    m_last, m_local = orb.ORBmatcher(0.9, True), orb.ORBmatcher(0.8, False)
    res = {}
    plan = lambda m: np.array([m.last_search_plan()[k] for k in PLAN_KEYS], np.int32)
    for cid in LAST_CASES:
        cur, last, mps, last_mp, last_outlier, lk = mc.pair_of(cid)
        g = np.full(cur.N, -1, np.int32)
        n = m_last.SearchByProjection_LastFrame(cur, g, last, lk, last_mp, last_outlier, mps, 15.0, True)
        res[f"last_{cid}_n"], res[f"last_{cid}_mp"], res[f"last_{cid}_plan"] = np.int32(n), g, plan(m_last)
    for cid, nq in LOCAL_CASES:
        pair = mc.pair_of(cid)
        in_view, px, pxr, py, level, view_cos, mp_index, cur_mp = local_queries(cid, nq)
        g = cur_mp.copy()
        n = m_local.SearchByProjection_MapPoints(pair[0], g, in_view, px, pxr, py, level, view_cos, mp_index, pair[2], 5.0)
        k = f"local_{cid}_{nq}"
        res[k + "_n"], res[k + "_mp"], res[k + "_plan"] = np.int32(n), g, plan(m_local)
    probs = mc.batch_problems(BATCH_NP)
    g = [p[2].copy() for p in probs]
    nm, nv = m_local.SearchLocalPoints([p[0][0] for p in probs], g, [p[1] for p in probs], mc.LOG_SCALE_FACTOR, 3.0)
    res["batch_nm"], res["batch_nv"], res["batch_plan"] = nm, nv, plan(m_local)
    for k, gk in enumerate(g):
        res[f"batch_mp{k}"] = gk
    np.savez(out, **res)
    print({k: v.tolist() for k, v in res.items() if k.endswith("_plan")}, flush=True)


if __name__ == "__main__":
    main()
