"""CPU: the numpy restatement of cv::remap (tests/remap_ref.py) pinned on values that follow from
the definitions, the case generator's EuRoC-shaped maps, and the binding / header declarations of
the new entry points with the argument errors they answer before any device work.

cv::remap: OpenCV 3.2's fixed-point INTER_LINEAR path (5 fraction bits, 15-bit weights, ties to even,
BORDER_CONSTANT 0); "parity unpinned" (OpenCV absent), as cvtColor in tests/test_rgbd_cpu.py."""
import ctypes as C
import re

import numpy as np

import remap_cases as cases
import remap_ref as ref
from c_orb_slam_amd import _lib

NEW = ["ORBextractor_set_remap", "ORBextractor_remap_batch"]


def _row(mx, my=0.0, src=None):
    src = np.array([[0, 20, 40, 60]], np.uint8) if src is None else src
    return int(ref.remap(src, np.full((1, 1), mx, np.float32), np.full((1, 1), my, np.float32))[0, 0])


def test_identity_map_reproduces_the_source():
    rng = np.random.default_rng(3)
    src = rng.integers(0, 256, (9, 13), dtype=np.uint8)
    xs, ys = cases.grid_maps(np.arange(13), np.arange(9))
    assert np.array_equal(ref.remap(src, xs, ys), src)
    # a shift by whole pixels moves the image and fills with 0
    out = ref.remap(src, xs + np.float32(2), ys - np.float32(1))
    assert np.array_equal(out[1:, :11], src[:8, 2:]) and not out[0].any() and not out[:, 11:].any()


def test_hand_worked_values():
    assert _row(2.984375) == 60        # x32 = 95.5, ties to even -> 96 = pixel 3 exactly
    assert _row(0.015625) == 0         # x32 = 0.5 -> 0
    assert _row(0.046875) == 1         # x32 = 1.5 -> 2: (0*30 + 20*2) * 32 * 32 -> 1.25 -> 1
    assert _row(-0.5) == 0             # ix = -1, fx = 16: half of pixel 0, which is 0
    assert _row(3.5) == 30             # ix = 3, fx = 16: half of 60, the tap at 4 is outside
    assert _row(-0.5, src=np.array([[200, 0, 0, 0]], np.uint8)) == 100
    for v in (np.nan, np.inf, -np.inf, 1e9, -1e9):
        assert _row(v) == 0 and _row(1.0, v) == 0
    assert _row(1.0) == 20 and _row(1.0, -1.0) == 0 and _row(1.0, 1.0) == 0 and _row(1.0, -0.5) == 10
    # ties on negative coordinates: -0.015625 * 32 = -0.5 -> -0 (even); -0.046875 * 32 = -1.5 -> -2
    ix, iy, fx, fy, valid = ref.quantise(np.array([[-0.015625, -0.046875, -1.0, 2.5e7, 4e7]], np.float32),
                                         np.zeros((1, 5), np.float32))
    assert ix[0, :3].tolist() == [0, -1, -1] and fx[0, :3].tolist() == [0, 30, 0]
    assert valid[0].tolist() == [True, True, True, True, False]     # 4e7 * 32 >= 2^30


def test_weights_sum_and_table_equivalence():
    fy, fx = np.divmod(np.arange(1024), 32)
    w = ref.weights(fx, fy)
    assert np.all(sum(w) == 32768)
    assert all(np.all(k >= 0) for k in w)
    # OpenCV's table entry is saturate_cast<short>(vy * vx * 32768) with float 5-bit ratios: the
    # closed form, except 32768 at fx = fy = 0 where it holds 32767 (+1 elsewhere in the block)
    one = np.float32(1)
    for i in range(1024):
        vx = (one - np.float32(fx[i]) / np.float32(32), np.float32(fx[i]) / np.float32(32))
        vy = (one - np.float32(fy[i]) / np.float32(32), np.float32(fy[i]) / np.float32(32))
        tab = [float(vy[a] * vx[b] * np.float32(32768)) for a in (0, 1) for b in (0, 1)]
        assert tab == [float(k[i]) for k in w]
    s00, s = np.meshgrid(np.arange(256, dtype=np.int64), np.arange(256, dtype=np.int64))
    assert np.array_equal((s00 * 32767 + s * 1 + 16384) >> 15, s00)     # (32767, 0, 0, 1) == (32768, 0, 0, 0)
    assert np.array_equal((s00 * 32768 + 16384) >> 15, s00)
    assert not ((s + 16384) >> 15).any()
    # the combination never exceeds 255
    assert (255 * 32768 + 16384) >> 15 == 255


def test_euroc_maps_reach_every_table_entry_and_stay_inside():
    for side in ("left", "right"):
        m1, m2 = cases.euroc_maps(side)
        assert m1.shape == m2.shape == (cases.H, cases.W) and m1.dtype == np.float32
        ix, iy, fx, fy, valid = ref.quantise(m1, m2)
        assert valid.all()
        assert len(np.unique(fy * 32 + fx)) == 1024, side
        assert ix.min() >= 0 and ix.max() + 1 < cases.W and iy.min() >= 0, side
        low = iy + 1 >= cases.H
        if side == "left":
            assert not low.any()               # every tap inside: the border cases are synthetic
        else:
            # the right camera's lowest rectified row dips to 479.18: these few pixels straddle the
            # bottom border with fy <= 6 (BORDER_CONSTANT gives their lower taps 0)
            assert 0 < low.sum() <= 64 and np.all(np.argwhere(low)[:, 0] == cases.H - 1)
            assert iy.max() == cases.H - 1 and fy[low].max() <= 6
        # neighbouring destination pixels are neighbours in the source
        assert np.abs(np.diff(m1, axis=1)).max() < 1.06
        assert (iy.max(axis=1) - iy.min(axis=1)).max() + 2 <= 40


def test_case_generators():
    m1, m2 = cases.table_maps()
    ix, iy, fx, fy, valid = ref.quantise(m1, m2)
    assert np.array_equal(fx, np.tile(np.arange(32), (32, 1))) and np.array_equal(fy, fx.T)
    assert np.all(ix == 3) and np.all(iy == 2)
    t = cases.tie_values()
    v = t.astype(np.float64) * 32
    assert np.all(np.abs(v - np.trunc(v)) == 0.5) and (t < 0).any() and (t > 0).any()
    sx = np.rint(t * np.float32(32)).astype(np.int64)
    assert np.all(sx % 2 == 0)                                    # ties go to even
    b = cases.border_values(7)
    ix = ref.quantise(b[None], np.zeros((1, len(b)), np.float32))[0][0]
    assert {-2, -1, 0, 5, 6, 7}.issubset(set(ix.tolist()))
    assert np.isnan(b).any() and np.isinf(b).any()
    rng = np.random.default_rng(4)
    r1, r2 = cases.random_maps(rng, 40, 30, 9, 5)
    assert r1.dtype == np.float32 and (r1 < 0).any() and (r1 > 9).any() and np.isnan(r1).any()
    s = cases.source(rng, 6, 8, 1)
    assert set(np.unique(s)) == {0, 255}
    p = cases.in_pitch(r1, 3)
    assert p.strides == (40 * 4 + 3, 4)
    assert np.array_equal(np.ascontiguousarray(p).view(np.uint8), r1.view(np.uint8))
    # the rendered raw image, rectified by the reference, is the scene again (up to two resamplings)
    u, v = np.meshgrid(np.arange(cases.W), np.arange(cases.H))
    scene = (128 + 100 * np.sin(u / 23.0) * np.cos(v / 17.0)).astype(np.uint8)
    raw = cases.render_raw(scene, "left")
    rect = ref.remap(raw, *cases.euroc_maps("left"))
    # away from the edges, where the scene outside the rendered field of view is missing
    assert np.abs(rect.astype(int) - scene.astype(int))[40:-40, 60:-60].max() <= 3
    assert np.abs(raw.astype(int) - scene.astype(int)).max() > 20       # the raw image is distorted


def test_bindings_and_header_declare_the_entries():
    names = _lib.header_functions()
    src = (_lib.PKG / "_lib.py").read_text()
    for n in NEW:
        assert n in names, n
        assert re.search(rf"L\.{n}\.argtypes", src), n
        assert hasattr(_lib.lib(), n), n
    hdr = _lib.HEADER.read_text()
    assert re.search(r"#define ORB_REMAP_SLOTS 4\b", hdr) and _lib.ORB_REMAP_SLOTS == 4
    assert re.search(r"#define ORBGPU_ABI_VERSION 2\b", hdr)            # entries were only added
    from c_orb_slam_amd.orb import ORBextractor
    for m in ("set_remap", "remap_device", "extract_rectified"):
        assert callable(getattr(ORBextractor, m))


def test_argument_errors_without_a_device():
    """Every listed argument error is ORB_E_INVALID before any device work.  No handle exists
    without a device, so these go through h == NULL, which answers as the neighbouring entries do;
    tests/test_gpu_remap.py repeats them on a live handle."""
    L = _lib.lib()
    inv = _lib.ORB_E_INVALID
    m = np.zeros((4, 4), np.float32)
    img = np.zeros((4, 4), np.uint8)
    mp, ip = _lib.ptr(m), _lib.ptr(img)
    assert L.ORBextractor_cvtColor_batch(None, None, 1, 4, 4, 3, 1, 12, 48, 0, None, 4, 16) == inv   # the neighbour
    assert L.ORBextractor_set_remap(None, 0, mp, mp, 4, 4, 16, 0) == inv
    assert L.ORBextractor_set_remap(None, 0, None, None, 0, 0, 0, 0) == inv
    assert L.ORBextractor_set_remap(None, -1, mp, mp, 4, 4, 16, 0) == inv
    assert L.ORBextractor_set_remap(None, _lib.ORB_REMAP_SLOTS, mp, mp, 4, 4, 16, 0) == inv
    assert L.ORBextractor_set_remap(None, 0, mp, None, 4, 4, 16, 0) == inv
    assert L.ORBextractor_set_remap(None, 0, mp, mp, 4, 4, 15, 0) == inv
    rb = L.ORBextractor_remap_batch
    assert rb(None, ip, 1, 4, 4, 4, 16, 0, 0, 1, ip, 4, 16) == inv
    assert rb(None, ip, 0, 4, 4, 4, 16, 0, 0, 1, ip, 4, 16) == inv       # h is checked before the empty batch
    assert rb(None, None, 1, 4, 4, 4, 16, 0, 0, 1, None, 4, 16) == inv
    assert rb(None, ip, 1, 4, 4, 4, 16, 0, 0, 0, ip, 4, 16) == inv       # slot_period < 1
    assert rb(None, ip, 1, 4, 4, 4, 16, 0, 3, 2, ip, 4, 16) == inv       # slot0 + slot_period > slots
    assert rb(None, ip, 1, 4, 4, 3, 16, 0, 0, 1, ip, 4, 16) == inv       # step below a row
    assert rb(None, ip, 65536, 4, 4, 4, 16, 0, 0, 1, ip, 4, 16) == inv
    assert rb(None, ip, -1, 4, 4, 4, 16, 0, 0, 1, ip, 4, 16) == inv
    assert C.sizeof(C.c_size_t) == 8
