"""The extractor's opt-in launch paths against the CPU oracle, bit for bit.

The library keeps several alternative schedules of the same arithmetic behind environment
variables: ORBGPU_FAST_SPLIT (FAST of the large levels on a side stream), ORBGPU_BLUR_SIDE
(the blur on a side stream), ORBGPU_PYR_FLOW (the pyramid as one launch of dependent tasks) are read
when an extractor is created; ORBGPU_PYR_CHAIN / ORBGPU_PYR_CHAIN_FROM (the small levels chained in
one launch) and ORBGPU_BLUR_EARLY are read once per process and so run in a fresh child process
(extract_path_worker.py), one at a time.  Every test first asserts, through
orbgpu_debug_extract_plan, that the path under test really ran: a plan that silently falls back to
the default launches must fail, not pass.  Two different batches go through one extractor, so a
result read before its producer finished would show the previous call's bytes.
"""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import extract_cases as ec
import extract_path_worker as worker
import oracle_lib

pytestmark = pytest.mark.gpu

WORKER = Path(__file__).resolve().parent / "extract_path_worker.py"
QVGA5 = (320, 240, 1.2, 5, 500)
VGA8 = (640, 480, 1.2, 8, 1000)
QVGA12 = (320, 240, 1.1, 12, 500)
ODD15 = (333, 217, 1.5, 4, 400)

_REF = {}


def _reference(case, img):
    """The oracle's outputs for one image, computed once per (case, image)."""
    W, H, sf, nl, nf = case
    key = (case, img.tobytes())
    if key not in _REF:
        orc = oracle_lib.OracleExtractor(nf, sf, nl, 20, 7)
        k, d = orc(img)
        _REF[key] = dict(kps=k, desc=d, levels=[orc.level(l) for l in range(nl)],
                         blur=[orc.blurred(l) for l in range(nl)])
    return _REF[key]


def _assert_equal(ref, levels, blur, kps, desc, nl, what):
    for l in range(nl):
        assert levels[l].shape == ref["levels"][l].shape, f"{what} level {l}"
        assert np.array_equal(levels[l], ref["levels"][l]), \
            f"{what} pyramid level {l} differs at {np.argwhere(levels[l] != ref['levels'][l])[:5]}"
    if blur is not None:
        for l in range(nl):
            assert np.array_equal(blur[l], ref["blur"][l]), \
                f"{what} blurred level {l} differs at {np.argwhere(blur[l] != ref['blur'][l])[:5]}"
    if kps is not None:
        ec.assert_keypoints_equal(kps, desc, ref["kps"], ref["desc"], nl, what)


def _two_batches(gpu, case, B, want_flags, mask):
    W, H, sf, nl, nf = case
    ex = gpu.ORBextractor(nf, sf, nl, 20, 7, max_width=W, max_height=H, max_batch=B)
    for call in range(worker.CALLS):
        imgs = worker.batch_images(W, H, B, call)
        res = ex.extract_batch(imgs)
        flags, chain_from, _ = ec.extract_plan(ex)
        assert flags & mask == want_flags and chain_from == 0, (flags, chain_from)
        for b in range(B):
            _assert_equal(_reference(case, imgs[b]), [ex.image_pyramid_level(l, b) for l in range(nl)],
                          [ex.blurred_level(l, b) for l in range(nl)], res[b][0], res[b][1], nl,
                          f"call {call} image {b}:")


PATH_VARS = ("ORBGPU_FAST_SPLIT", "ORBGPU_BLUR_SIDE", "ORBGPU_PYR_FLOW", "ORBGPU_PYR_CHAIN", "ORBGPU_PYR_CHAIN_FROM",
             "ORBGPU_BLUR_EARLY")
ALL_PATHS = ec.PLAN_FLOW | ec.PLAN_CHAIN | ec.PLAN_FAST_SPLIT | ec.PLAN_BLUR_SIDE | ec.PLAN_BLUR_EARLY


@pytest.mark.parametrize("B", [1, 8])
@pytest.mark.parametrize("case", [QVGA5, VGA8], ids=ec.case_id)
@pytest.mark.parametrize("var,flag", [("ORBGPU_FAST_SPLIT", ec.PLAN_FAST_SPLIT), ("ORBGPU_BLUR_SIDE", ec.PLAN_BLUR_SIDE)])
def test_side_stream_paths(gpu, monkeypatch, var, flag, case, B):
    for v in ("ORBGPU_FAST_SPLIT", "ORBGPU_BLUR_SIDE", "ORBGPU_PYR_FLOW"):
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setenv(var, "1")
    _two_batches(gpu, case, B, flag, ALL_PATHS)


@pytest.mark.parametrize("B", [3, 8])
@pytest.mark.parametrize("case", [QVGA5, ODD15], ids=ec.case_id)
def test_pyramid_flow_small_levels(gpu, monkeypatch, case, B):
    """k_pyr_flow on levels of a few tiles and bands (and, at scale 1.5, source rectangles of
    several staging rounds): padded levels over alternating batches, as at KITTI size in
    test_gpu_extract.py, and everything built on them."""
    for v in ("ORBGPU_FAST_SPLIT", "ORBGPU_BLUR_SIDE"):
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setenv("ORBGPU_PYR_FLOW", "1")
    W, H, sf, nl, nf = case
    ex = gpu.ORBextractor(nf, sf, nl, 20, 7, max_width=W, max_height=H, max_batch=B)
    first, second = worker.batch_images(W, H, B, 0), worker.batch_images(W, H, B, 1)
    for s, imgs in enumerate([first, second, first[::-1], second[: max(1, B // 2)]]):
        res = ex.extract_batch(np.ascontiguousarray(imgs))
        flags, chain_from, _ = ec.extract_plan(ex)
        assert flags & ALL_PATHS == ec.PLAN_FLOW and chain_from == 0, (flags, chain_from)
        for b, img in enumerate(imgs):
            _assert_equal(_reference(case, img), [ex.image_pyramid_level(l, b) for l in range(nl)],
                          [ex.blurred_level(l, b) for l in range(nl)], res[b][0], res[b][1], nl,
                          f"set {s} image {b}:")


def _run_worker(tmp_path, case, B, env_vars):
    W, H, sf, nl, nf = case
    out = tmp_path / "result.npz"
    env = {k: v for k, v in os.environ.items() if k not in PATH_VARS}
    env.update(env_vars)
    p = subprocess.run([sys.executable, str(WORKER), str(W), str(H), str(sf), str(nl), str(nf), str(B), str(out)],
                       env=env, timeout=120, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-4000:]
    return np.load(out)


def _check_worker(z, case, B, want_flags, want_from):
    W, H, sf, nl, nf = case
    for call in range(worker.CALLS):
        flags, chain_from = z[f"c{call}_plan"]
        assert flags & ALL_PATHS == want_flags and chain_from == want_from, (call, flags, chain_from)
        imgs = worker.batch_images(W, H, B, call)
        for b in range(B):
            p = f"c{call}_b{b}_"
            _assert_equal(_reference(case, imgs[b]), [z[p + f"level{l}"] for l in range(nl)],
                          [z[p + f"blur{l}"] for l in range(nl)], z[p + "kps"], z[p + "desc"], nl,
                          f"call {call} image {b}:")


@pytest.mark.parametrize("case,B,chain_from", [(VGA8, 1, 3), (VGA8, 8, 3), (QVGA12, 1, 3), (QVGA12, 8, 3), (VGA8, 1, 2),
                                               (VGA8, 8, 2)],
                         ids=lambda v: ec.case_id(v) if isinstance(v, tuple) else str(v))
def test_pyramid_chain(gpu, tmp_path, case, B, chain_from):
    """k_pyr_chain / plan_chain: levels [chain_from, nlevels) of every image in one launch."""
    env = {"ORBGPU_PYR_CHAIN": "1"}
    if chain_from != 3:
        env["ORBGPU_PYR_CHAIN_FROM"] = str(chain_from)
    z = _run_worker(tmp_path, case, B, env)
    _check_worker(z, case, B, ec.PLAN_CHAIN, chain_from)


@pytest.mark.parametrize("B", [1, 8])
def test_blur_early(gpu, tmp_path, B):
    z = _run_worker(tmp_path, QVGA5, B, {"ORBGPU_BLUR_EARLY": "1"})
    _check_worker(z, QVGA5, B, ec.PLAN_BLUR_EARLY, 0)
