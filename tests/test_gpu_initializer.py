"""GPU: Initializer_Initialize against the scalar restatement (tests/initializer_ref.py), bit for
bit: ok, R21, t21, vP3D, vbTriangulated, every orb_init_info field and both inlier masks.  A NaN
parallax (acos of a cosine that rounded above 1) equals any NaN; everything else is compared by
bit pattern."""
import ctypes as C
import threading

import numpy as np
import pytest

import initializer_cases as ic
import initializer_ref as ir
from c_orb_slam_amd._lib import ORB_E_INVALID, lib, orb_init_info, ptr
from c_orb_slam_amd.ransac import Initializer, Rng

pytestmark = pytest.mark.gpu

# (kind, seed, N, outlier share, iterations, scene keywords).  N = 8 makes every set a
# permutation of all matches; 63 / 64 / 65 straddle a wave; 300 spans several score chunks and
# more than one CheckRT stride.
CASES = [
    ("general", 3, 8, 0.0, 1, {}),
    ("general", 2, 9, 0.3, 7, {}),
    ("general", 1, 63, 0.0, 32, {}),
    ("general", 2, 64, 0.3, 7, {}),
    ("general", 1, 65, 0.0, 1, {}),
    ("general", 1, 300, 0.0, 32, {}),
    ("general", 1, 300, 0.3, 32, {}),
    ("general", 1, 24, 0.0, 200, {}),
    ("planar", 1, 300, 0.0, 32, {}),
    ("planar", 1, 300, 0.3, 32, {}),
    ("planar", 2, 64, 0.0, 7, {}),
    ("rotation", 1, 300, 0.0, 32, {}),
    ("rotation", 1, 300, 0.3, 32, {}),
    ("rotation", 1, 64, 0.0, 7, {"noise": 0.0}),
    ("low_parallax", 1, 300, 0.0, 32, {}),
    ("low_parallax", 1, 300, 0.3, 32, {}),
    ("low_parallax", 1, 65, 0.0, 32, {}),
    ("low_parallax", 3, 65, 0.0, 32, {}),
    ("low_parallax", 3, 64, 0.3, 32, {"tiny": True}),
    ("few_good", 1, 63, 0.0, 32, {}),
    ("few_good", 1, 65, 0.3, 7, {}),
]
_IDS = [f"{k}-s{s}-N{n}-o{o}-it{it}" + ("-" + "-".join(kw) if kw else "") for k, s, n, o, it, kw in CASES]
_restated = {}


def _scene(case):
    kind, seed, N, outl, _, kw = case
    return ic.scene(kind, seed, N, outl, **kw)


def restated(case, seed=0):
    """The restatement's result of one case (cached per module) and the draws it consumed."""
    key = (CASES.index(case), seed)
    if key not in _restated:
        s = _scene(case)
        g = ir.GlibcRand(seed)
        r = ir.Initializer(s["K"], s["keys1"], 1.0, case[4]).Initialize(s["keys2"], s["matches12"], g)
        _restated[key] = (r, g.count)
    return _restated[key]


def _bits(a, dtype=np.float32):
    return np.ascontiguousarray(a, dtype).view(np.uint32 if dtype == np.float32 else np.uint8)


def _same_floats(a, b):
    a, b = np.asarray(a, np.float32).ravel(), np.asarray(b, np.float32).ravel()
    nan = np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and bool(np.all(nan | (a.view(np.uint32) == b.view(np.uint32))))


def assert_equal(dev, ref, what=""):
    ok, R, t, P3D, tri, info = dev
    rinfo = ref["info"]
    assert ok == ref["ok"], what
    if info is not None:
        for k in ("use_H", "best_it_H", "best_it_F", "n_hyp", "chosen"):
            assert info[k] == rinfo[k], (what, k, info[k], rinfo[k])
        assert info["nGood"] == rinfo["nGood"], (what, info["nGood"], rinfo["nGood"])
        for k in ("SH", "SF", "H21", "F21", "parallax"):
            assert _same_floats(info[k], rinfo[k]), (what, k, info[k], rinfo[k])
        assert np.array_equal(info["inliersH"], rinfo["inliersH"]), what
        assert np.array_equal(info["inliersF"], rinfo["inliersF"]), what
    if ok:
        assert _same_floats(R, ref["R21"]) and _same_floats(t, ref["t21"]), (what, R, ref["R21"], t, ref["t21"])
        assert np.array_equal(tri, ref["vbTriangulated"]), what
        assert np.array_equal(_bits(P3D), _bits(ref["vP3D"])), what


def _run(case, seed=0, want_info=True):
    s = _scene(case)
    g = Rng(seed)
    I = Initializer(s["K"], s["keys1"], 1.0, case[4])
    out = I.Initialize(s["keys2"], s["matches12"], g, want_info=want_info)
    I.close()
    return out, g


def _advanced(seed, draws):
    g = Rng(seed)
    for _ in range(draws):
        g.rand()
    return g.state()


@pytest.mark.parametrize("case", CASES, ids=_IDS)
def test_device_equals_restatement(gpu, case):
    ref, draws = restated(case)
    out, g = _run(case)
    assert_equal(out, ref, case)
    assert draws == 8 * case[4] and g.state() == _advanced(0, draws)


def test_cases_reach_every_branch():
    """Across the cases: both branches of RH, an H and an F success, and failures by nsimilar > 1,
    by the d1/d2 gate and by parallax."""
    seen = set()
    for case in CASES:
        r, _ = restated(case)
        info = r["info"]
        seen.add("H" if info["use_H"] else "F")
        seen.add(("ok" if r["ok"] else "fail:" + info["why"]) + (" H" if info["use_H"] else " F"))
    print(sorted(seen))
    for want in ("H", "F", "ok H", "ok F", "fail:nsimilar F", "fail:gate H"):
        assert want in seen, (want, sorted(seen))
    assert "fail:parallax F" in seen or "fail:parallax H" in seen, sorted(seen)


def test_two_calls_share_one_stream(gpu):
    """Two Initialize calls on one handle with different current frames and one continuing rng
    equal two restatement calls; the stream ends 16 * iterations draws on."""
    its = 7
    a = ic.scene("general", 5, 64, 0.0)
    b = ic.scene("general", 6, 64, 0.3, extra=(7, 9))      # another current frame: n2 differs, other holes
    g, rg = Rng(0), ir.GlibcRand(0)
    I = Initializer(a["K"], a["keys1"], 1.0, its)
    R = ir.Initializer(a["K"], a["keys1"], 1.0, its)
    for keys2, m in ((a["keys2"], a["matches12"]), (b["keys2"], b["matches12"])):
        assert_equal(I.Initialize(keys2, m, g), R.Initialize(keys2, m, rg), "shared stream")
    I.close()
    assert rg.count == 16 * its and g.state() == _advanced(0, 16 * its)


@pytest.mark.parametrize("case", [CASES[5], CASES[8], CASES[11]], ids=["F-success", "H-success", "failure"])
def test_null_info_gives_the_same_outputs(gpu, case):
    ref, _ = restated(case)
    out, _ = _run(case, want_info=False)
    assert out[5] is None
    assert_equal(out, ref, case)
    # info without the two masks
    s = _scene(case)
    L, g = lib(), Rng(0)
    I = Initializer(s["K"], s["keys1"], 1.0, case[4])
    n1 = len(s["keys1"])
    R, t, P, tri = np.zeros(9, np.float32), np.zeros(3, np.float32), np.zeros((n1, 3), np.float32), np.zeros(n1, np.uint8)
    ok, info = C.c_int(), orb_init_info()
    assert L.Initializer_Initialize(I._h, len(s["keys2"]), ptr(s["keys2"]), ptr(s["matches12"]), C.byref(g.s), ptr(R),
                                    ptr(t), ptr(P), ptr(tri), C.byref(ok), C.byref(info)) == 0
    I.close()
    assert bool(ok.value) == ref["ok"] and info.chosen == ref["info"]["chosen"]
    if ref["ok"]:
        assert _same_floats(R, ref["R21"]) and np.array_equal(_bits(P), _bits(ref["vP3D"]))


def test_failure_leaves_the_outputs_untouched_and_bad_matches_are_rejected(gpu):
    case = CASES[11]                                     # pure rotation: fails
    assert not restated(case)[0]["ok"]
    s = _scene(case)
    L, g = lib(), Rng(0)
    I = Initializer(s["K"], s["keys1"], 1.0, case[4])
    n1, n2 = len(s["keys1"]), len(s["keys2"])
    R, t = np.full(9, 7.5, np.float32), np.full(3, 7.5, np.float32)
    P, tri = np.full((n1, 3), 7.5, np.float32), np.full(n1, 9, np.uint8)
    ok = C.c_int(5)

    def call(m12, nn2=n2):
        return L.Initializer_Initialize(I._h, nn2, ptr(s["keys2"]), ptr(m12), C.byref(g.s), ptr(R), ptr(t), ptr(P),
                                        ptr(tri), C.byref(ok), None)

    assert call(s["matches12"]) == 0 and ok.value == 0
    assert np.all(R == 7.5) and np.all(t == 7.5) and np.all(P == 7.5) and np.all(tri == 9)
    # argument errors that need the handle's n1: a match index outside [0, n2), fewer than 8 matches
    before = g.state()
    bad = s["matches12"].copy()
    bad[np.nonzero(bad >= 0)[0][0]] = n2
    assert call(bad) == ORB_E_INVALID
    few = np.full(n1, -1, np.int32)
    few[:7] = np.arange(7)
    assert call(few) == ORB_E_INVALID
    assert g.state() == before
    I.close()


def test_two_handles_on_two_threads(gpu):
    cases = [CASES[5], CASES[8]]
    outs = [None, None]

    def work(k):
        for _ in range(3):
            outs[k] = _run(cases[k])[0]

    ths = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for th in ths:
        th.start()
    for th in ths:
        th.join()
    for k in range(2):
        assert_equal(outs[k], restated(cases[k])[0], ("thread", k))
        assert_equal(_run(cases[k])[0], restated(cases[k])[0], ("serial", k))


def test_chain_from_search_for_initialization(gpu):
    """ORBmatcher_SearchForInitialization's vnMatches12 of two extracted synthetic frames goes
    straight into Initialize and equals the restatement."""
    import search_cases as sc
    (k0, d0), (k1, d1) = sc.frames(0)[0]
    t = sc.frames(0)[3]
    F1 = sc.make_frame(k0, d0, t, np.eye(4, dtype=np.float32))
    F2 = sc.make_frame(k1, d1, t, np.eye(4, dtype=np.float32))
    keys1 = np.ascontiguousarray(np.stack([k0["x"], k0["y"]], 1), np.float32)
    keys2 = np.ascontiguousarray(np.stack([k1["x"], k1["y"]], 1), np.float32)
    n, m12 = gpu.ORBmatcher(0.9, True).SearchForInitialization(F1, F2, keys1.copy(), 100)
    assert n >= 100
    its = 16
    g, rg = Rng(0), ir.GlibcRand(0)
    I = Initializer(ic.K, keys1, 1.0, its)
    out = I.Initialize(keys2, m12, g)
    I.close()
    assert_equal(out, ir.Initializer(ic.K, keys1, 1.0, its).Initialize(keys2, m12, rg), "chain")
    assert g.state() == _advanced(0, 8 * its)
