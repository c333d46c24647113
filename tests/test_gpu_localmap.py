"""LocalMapping_CreateNewMapPoints_batch and MapPoint_Update_batch on the GPU against the scalar
restatement (tests/localmap_ref.py), bit for bit on every pair and point: status, x3D, normal,
max_dist, min_dist, best."""
import ctypes as C

import numpy as np
import pytest

import localmap_cases as lc
import localmap_ref as lr

pytestmark = pytest.mark.gpu


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _assert_outputs(got, want, what):
    assert len(got) == len(want), what
    for j, (g, w) in enumerate(zip(got, want)):
        for name, ga, wa in zip(("x3D", "status", "normal", "max_dist", "min_dist"), g, w):
            if not _same(ga, wa):
                rows = lambda a: np.ascontiguousarray(a).reshape(len(a), -1).view(np.uint8)   # noqa: E731
                bad = np.flatnonzero((rows(ga) != rows(wa)).any(axis=1))[:5]
                raise AssertionError((what, j, name, bad, ga[bad], wa[bad], g[1][bad], w[1][bad]))


@pytest.mark.parametrize("kind", ["sideways", "forward"])
@pytest.mark.parametrize("stereo_frac", [0.0, 0.5, 1.0])
def test_create_new_map_points(gpu, kind, stereo_frac):
    m = gpu.ORBmatcher(0.6, True)
    seen = set()
    for npairs in (1, 63, 64, 65, 600):
        s = lc.scene(kind, stereo_frac, npairs)
        args = (s["KF1"], s["depth1"], s["sigma2"], s["scaleFactor"], lc.neighbours_of(s))
        got = m.CreateNewMapPoints(*args)
        want = lr.restate_batch(*args)
        _assert_outputs(got, want, (kind, stereo_frac, npairs))
        seen |= set(int(v) for v in got[0][1])
        # without the optional outputs: the same points
        (x3D, status, normal, _, _), = m.CreateNewMapPoints(*args, want_normal=False)
        assert _same(x3D, want[0][0]) and _same(status, want[0][1]) and not normal.any()
    if kind == "sideways":
        assert {1, -2, -3, -5, -7} <= seen, seen
    else:
        assert (0 in seen) if stereo_frac == 0 else (2 in seen), seen


@pytest.mark.parametrize("kind,stereo_frac", [("sideways", 0.5), ("forward", 1.0)])
def test_create_new_map_points_batch_of_neighbours(gpu, kind, stereo_frac):
    """Three neighbours, the middle one without pairs, in one call; the same three as single
    calls give identical bytes; a call without neighbours is a no-op."""
    m = gpu.ORBmatcher(0.6, True)
    base, nbs = lc.multi_scene(kind, stereo_frac, [130, 0, 97])
    head = (base["KF1"], base["depth1"], base["sigma2"], base["scaleFactor"])
    got = m.CreateNewMapPoints(*head, nbs)
    want = lr.restate_batch(*head, nbs)
    _assert_outputs(got, want, "batch")
    assert len(got[1][1]) == 0
    singles = [m.CreateNewMapPoints(*head, [nb])[0] for nb in nbs]
    _assert_outputs(singles, got, "single calls")
    assert sum(int((g[1] > 0).sum()) for g in got) >= 20
    assert m.CreateNewMapPoints(*head, []) == []


@pytest.mark.parametrize("seed,stereo_frac", [(0, 0.0), (8, 0.5)])
def test_search_for_triangulation_feeds_create_new_map_points(gpu, seed, stereo_frac):
    """The chain LocalMapping runs: the pairs of ORBmatcher.SearchForTriangulation on extracted
    frames go straight into CreateNewMapPoints."""
    import search_cases as sc
    from c_orb_slam_amd import synthetic
    (k0, d0), (k1, d1) = sc.frames(seed)[0]
    t = sc.frames(seed)[3]
    rng = np.random.default_rng(seed + 2)
    T1, T2 = np.eye(4, dtype=np.float32), np.eye(4, dtype=np.float32)
    T2[:3, :3] = synthetic.small_rotation(rng, 718.856)
    T2[:3, 3] = [-0.5, 0.02, -0.1]
    stereo = stereo_frac > 0
    uR1 = np.where(rng.random(len(k0)) < stereo_frac, k0["x"] - 20, -1).astype(np.float32)
    uR2 = np.where(rng.random(len(k1)) < stereo_frac, k1["x"] - 20, -1).astype(np.float32)
    KF1 = sc.make_frame(k0, d0, t, T1, uRight=uR1 if stereo else None)
    KF2 = sc.make_frame(k1, d1, t, T2, uRight=uR2 if stereo else None)
    dep1 = np.where(uR1 >= 0, KF1.bf / np.float32(20), np.float32(-1)).astype(np.float32) if stereo else None
    dep2 = np.where(uR2 >= 0, KF2.bf / np.float32(20), np.float32(-1)).astype(np.float32) if stereo else None
    R12 = T1[:3, :3] @ T2[:3, :3].T
    t12 = -R12 @ T2[:3, 3] + T1[:3, 3]
    fx, fy, cx, cy = synthetic.intrinsics(sc.W, sc.H)
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]])
    F12 = (np.linalg.inv(K).T @ sc.skew(t12) @ R12 @ np.linalg.inv(K)).astype(np.float32)
    none = np.zeros(len(k0), np.uint8), np.zeros(len(k1), np.uint8)
    m = gpu.ORBmatcher(0.6, False)
    pairs = m.SearchForTriangulation(KF1, none[0], sc.featvec(d0), KF2, none[1], sc.featvec(d1), t["sigma2"], F12)
    assert len(pairs) > 10
    args = (KF1, dep1, t["sigma2"], np.float32(1.2), [(KF2, dep2, t["sigma2"], pairs)])
    got = m.CreateNewMapPoints(*args)
    _assert_outputs(got, lr.restate_batch(*args), "chain")


def _restate_update(c):
    st = c["obs_start"]
    n = len(st) - 1
    best = np.full(n, -1, np.int32)
    normal, mx, mn = np.zeros((n, 3), np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32)
    for p in range(n):
        best[p] = lr.restate_best(c["obs_desc"][st[p]:st[p + 1]])
        if st[p + 1] > st[p]:
            normal[p], mx[p], mn[p] = lr.restate_normal_depth(c["pos"][p], c["obs_Ow"][st[p]:st[p + 1]], c["ref_Ow"][p],
                                                              c["ref_scale"][p], c["ref_scale_top"][p])
    return dict(best=best, normal=normal, max_dist=mx, min_dist=mn)


def _with_ties(c, ks):
    """Overwrite the descriptors of one point per hand-made tie set (the first unused point with
    that many observations)."""
    st, used = c["obs_start"], set()
    for d in lc.tie_descriptors().values():
        p = next((p for p, k in enumerate(ks) if k == len(d) and p not in used), None)
        if p is not None:
            used.add(p)
            c["obs_desc"][st[p]:st[p + 1]] = d
    return c


UPDATE_KS = {
    "mixed": [0, 1, 2, 3, 63, 64, 65, 130, 1025, 7, 4, 3, 2, 0],
    "one": [5],
    "npts257": [int(k) for k in np.random.default_rng(1).integers(0, 13, 257)],
}


@pytest.mark.parametrize("name", list(UPDATE_KS))
def test_map_point_update(gpu, name):
    ks = UPDATE_KS[name]
    c = _with_ties(lc.update_case(ks), ks)
    want = _restate_update(c)
    m = gpu.ORBmatcher(0.6, True)
    got = m.UpdateMapPoints(**c)
    for key in ("best", "normal", "max_dist", "min_dist"):
        assert _same(got[key], want[key]), (name, key, got[key][:16], want[key][:16])
    # only the descriptor part, only the normal part
    only_d = m.UpdateMapPoints(c["obs_start"], obs_desc=c["obs_desc"])
    assert set(only_d) == {"best"} and _same(only_d["best"], want["best"])
    only_n = m.UpdateMapPoints(c["obs_start"], pos=c["pos"], obs_Ow=c["obs_Ow"], ref_Ow=c["ref_Ow"],
                               ref_scale=c["ref_scale"], ref_scale_top=c["ref_scale_top"])
    assert set(only_n) == {"normal", "max_dist", "min_dist"}
    assert all(_same(only_n[k], want[k]) for k in only_n)
    if name == "mixed":
        assert want["best"][0] == -1 and want["best"][1] == 0 and want["best"][2] == 0
        assert (want["best"][3:9] > 0).any()


def test_single_observation_equals_create_stereo(gpu):
    """For k = 1 the point update is what MapPoint_CreateStereo_batch_device computes for a new
    stereo point: normal, max_dist and min_dist agree bit for bit."""
    import torch
    from c_orb_slam_amd._lib import KP_DTYPE, lib, orb_newpoints
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(4)
    n = 300
    k = np.zeros(n, KP_DTYPE)
    k["x"], k["y"] = rng.uniform(0, lc.W, n), rng.uniform(0, lc.H, n)
    k["octave"] = rng.integers(0, 8, n)
    dep = rng.uniform(0.5, 60, n).astype(np.float32)
    Twc = np.eye(4, dtype=np.float32)
    Twc[:3, :3] = lc.rodrigues(rng.normal(0, 0.2, 3))
    Twc[:3, 3] = rng.normal(0, 3, 3)
    scale, _ = lc.pyramid()
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)   # noqa: E731
    dk, dd, dT, ds = t(k.view(np.int32).reshape(n, 7)), t(dep), t(Twc.reshape(16)), t(scale)
    X = torch.zeros((n, 3), device=dev)
    row = torch.zeros(n, dtype=torch.int32, device=dev)
    nrm, mx, mn = torch.zeros((n, 3), device=dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    m = gpu.ORBmatcher(0.8, False)
    q = orb_newpoints(n, dk.data_ptr(), dd.data_ptr(), dT.data_ptr(), lc.FX, lc.FY, lc.CX, lc.CY, ds.data_ptr(), 8, 0,
                      X.data_ptr(), row.data_ptr(), nrm.data_ptr(), mx.data_ptr(), mn.data_ptr())
    assert lib().MapPoint_CreateStereo_batch_device(m._h, 1, C.byref(q)) == 0
    torch.cuda.synchronize()
    Ow = np.tile(Twc[:3, 3], (n, 1))
    got = m.UpdateMapPoints(np.arange(n + 1, dtype=np.int32), pos=X.cpu().numpy(), obs_Ow=Ow, ref_Ow=Ow,
                            ref_scale=scale[k["octave"]], ref_scale_top=np.full(n, scale[7], np.float32))
    assert _same(got["normal"], nrm.cpu().numpy())
    assert _same(got["max_dist"], mx.cpu().numpy()) and _same(got["min_dist"], mn.cpu().numpy())


def test_device_pointer_mode_is_refused(gpu):
    from c_orb_slam_amd._lib import ORB_E_INVALID, OrbGpuError, lib
    m = gpu.ORBmatcher(0.6, True)
    lib().ORBmatcher_set_device_pointers(m._h, 1)
    s = lc.scene("sideways", 0.5, 63)
    with pytest.raises(OrbGpuError) as ei:
        m.CreateNewMapPoints(s["KF1"], s["depth1"], s["sigma2"], s["scaleFactor"], lc.neighbours_of(s))
    assert ei.value.code == ORB_E_INVALID
    with pytest.raises(OrbGpuError) as ei:
        m.UpdateMapPoints(**lc.update_case([1, 2, 3]))
    assert ei.value.code == ORB_E_INVALID
