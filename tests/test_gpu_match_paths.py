"""The guided matcher's environment-selected instantiations against the CPU oracle, bit for bit.

ORBGPU_CAND_NT=256 (k_candidates<*, true, 256>: the staged candidate search in 256-thread
workgroups), ORBGPU_SELECT_LOCAL_NT=512 (k_select_r<false, 512, 8>) and ORBGPU_CAND_LOCAL_STAGE=0
(the local search unstaged at any frame size) are A/B switches of DESIGN.md §6 that the library
reads once per process, so each setting runs tests/match_path_worker.py in a fresh child.  The
plan the child reports (ORBmatcher_last_search_plan) must show the instantiation under test: a
misspelt or ignored variable fails here instead of passing on the default launches.
"""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import match_cases as mc
import match_path_worker as worker
import oracle_lib

pytestmark = pytest.mark.gpu

WORKER = Path(__file__).resolve().parent / "match_path_worker.py"
PATH_VARS = ("ORBGPU_CAND_NT", "ORBGPU_SELECT_LOCAL_NT", "ORBGPU_CAND_LOCAL_STAGE")
ENVS = {
    "cand256": {"ORBGPU_CAND_NT": "256"},
    "select512": {"ORBGPU_SELECT_LOCAL_NT": "512"},
    "local-unstaged": {"ORBGPU_CAND_LOCAL_STAGE": "0"},
    "all": {"ORBGPU_CAND_NT": "256", "ORBGPU_SELECT_LOCAL_NT": "512", "ORBGPU_CAND_LOCAL_STAGE": "0"},
}

_REF = {}


def _reference():
    """The oracle's results for the worker's case list, computed once."""
    if _REF:
        return _REF
    for cid in worker.LAST_CASES:
        cur, last, mps, last_mp, last_outlier, lk = mc.pair_of(cid)
        o = np.full(cur.N, -1, np.int32)
        n = oracle_lib.oracle_search_last(cur, o, last, lk, last_mp, last_outlier, mps, 15.0, True, 0.9, True)
        _REF[f"last_{cid}"] = (n, o, cur.N, last.N)
    for cid, nq in worker.LOCAL_CASES:
        pair = mc.pair_of(cid)
        in_view, px, pxr, py, level, view_cos, mp_index, cur_mp = worker.local_queries(cid, nq)
        o = cur_mp.copy()
        n = oracle_lib.oracle_search_local(pair[0], o, pair[2].obs, in_view, px, pxr, py, level, view_cos,
                                           pair[2].desc[mp_index], mp_index, 5.0, 0.8)
        _REF[f"local_{cid}_{nq}"] = (n, o, pair[0].N, nq)
    probs = mc.batch_problems(worker.BATCH_NP)
    ref = []
    for pair, M, cm in probs:
        o = cm.copy()
        ref.append(oracle_lib.oracle_search_local_points(pair[0], o, M, mc.LOG_SCALE_FACTOR, 3.0, 0.8) + (o,))
    _REF["batch"] = ref
    return _REF


@pytest.mark.parametrize("name", list(ENVS))
def test_matcher_paths(gpu, tmp_path, name):
    env_vars = ENVS[name]
    out = tmp_path / "result.npz"
    env = {k: v for k, v in os.environ.items() if k not in PATH_VARS}
    env.update(env_vars)
    p = subprocess.run([sys.executable, str(WORKER), str(out)], env=env, timeout=180, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-4000:]
    z = np.load(out)
    ref = _reference()
    cand = 256 if "ORBGPU_CAND_NT" in env_vars else 1024
    select = 512 if "ORBGPU_SELECT_LOCAL_NT" in env_vars else 1024
    local_staged = "ORBGPU_CAND_LOCAL_STAGE" not in env_vars

    def check(key, want_plan):
        n, o = ref[key][:2]
        assert int(z[key + "_n"]) == n, (key, int(z[key + "_n"]), n)
        assert np.array_equal(z[key + "_mp"], o), (key, np.nonzero(z[key + "_mp"] != o)[0][:10])
        assert dict(zip(worker.PLAN_KEYS, z[key + "_plan"].tolist())) == want_plan, (key, z[key + "_plan"], want_plan)

    for cid in worker.LAST_CASES:        # LastFrame stays staged whatever the local switch says; 512-thread selection
        _, _, n_cur, n_last = ref[f"last_{cid}"]
        check(f"last_{cid}", dict(staged=1, cand_threads=cand, select_threads=512, max_n=n_cur, max_q=n_last, np=1))
    for cid, nq in worker.LOCAL_CASES:
        n_cur = ref[f"local_{cid}_{nq}"][2]
        check(f"local_{cid}_{nq}", dict(staged=int(local_staged), cand_threads=cand if local_staged else 256,
                                        select_threads=select, max_n=n_cur, max_q=nq, np=1))
    probs = mc.batch_problems(worker.BATCH_NP)
    want = dict(staged=int(local_staged), cand_threads=cand if local_staged else 256, select_threads=select,
                max_n=max(p[0][0].N for p in probs), max_q=max(len(p[1]["pos"]) for p in probs), np=worker.BATCH_NP)
    assert dict(zip(worker.PLAN_KEYS, z["batch_plan"].tolist())) == want, (z["batch_plan"], want)
    for k, (no, nvo, o) in enumerate(ref["batch"]):
        assert (int(z["batch_nm"][k]), int(z["batch_nv"][k])) == (no, nvo), k
        assert np.array_equal(z[f"batch_mp{k}"], o), k
    assert sum(r[0] > 0 for r in ref["batch"]) >= 2 and ref["local_mix-300_4700"][0] > 50
