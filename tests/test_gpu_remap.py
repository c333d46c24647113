"""The EuRoC stereo rectification on the GPU vs its numpy restatement (tests/remap_ref.py), byte for
byte: ORBextractor_set_remap + ORBextractor_remap_batch = cv::remap(src, dst, map1, map2,
cv::INTER_LINEAR) with BORDER_CONSTANT 0.

* geometries: destination widths 1-67 (around the 4-pixel quad and the 64-lane wave) by heights 1-5,
  sources of other sizes down to 1 x 1, padded step / dst_step / map_step, a destination one byte off
  its allocation, sentinel bytes around every destination row, the source as a window inside an
  array of 255s (a tap that reads a neighbour instead of 0 changes a byte), host and device sources
  and maps;
* maps: all 1024 (fx, fy) table entries, every tie k + 0.5 in 1/32 units with both signs, coordinates
  in [-2, 0), ix in {-1, W-1} and iy in {-1, H-1} with the corners, fully outside on each side, NaN,
  +-inf, +-1e9, on sources of 0 and 255 next to each other;
* batches: slot_period 1 and 2, slot0 > 0, a batch of 5 through 2 slots, unequal slots refused;
* ordering: remap, set_remap on the same slot, remap again with no wait in between;
* a 752 x 480 EuRoC-shaped stereo pair end to end: remap_batch (slot_period 2) -> extract_batch on
  the same handle, no wait in between; keypoints and descriptors equal the oracle's on the
  reference-rectified images, and extract_rectified returns the same.

cv::remap is "parity unpinned" (OpenCV absent); its restatement is pinned on CPU by
tests/test_remap_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib
import remap_cases as cases
import remap_ref as ref
from c_orb_slam_amd import synthetic
from c_orb_slam_amd._lib import ORB_E_INVALID, ORB_REMAP_SLOTS, lib

pytestmark = pytest.mark.gpu

SENT = 0xCD


@pytest.fixture(scope="module")
def ex(gpu):
    return gpu.ORBextractor(1200, 1.2, 8, 20, 7, max_width=cases.W, max_height=cases.H, max_batch=2)


def _dev():
    import torch
    return torch.device("cuda", 0)


def _set(ex, slot, m1, m2, on_device=False, extra=0, keep=None):
    """set_remap from host or device maps with `extra` bytes of row padding."""
    import torch
    p1, p2 = cases.in_pitch(m1, extra), cases.in_pitch(m2, extra)
    if not on_device:
        ex.set_remap(slot, p1, p2)
        return
    h, w = m1.shape
    step = p1.strides[0]
    d1 = torch.from_numpy(p1.base).to(_dev())   # in_pitch's byte buffer: h rows of step bytes
    d2 = torch.from_numpy(p2.base).to(_dev())
    torch.cuda.synchronize()
    keep.extend([d1, d2])   # the caller keeps them until the stream has passed the quantisation
    ex.set_remap_device(slot, d1.data_ptr(), d2.data_ptr(), w, h, step)


def _run(ex, imgs, dw, dh, slot0, period, step_extra=0, dstep_extra=0, off=0, on_device=True):
    """remap_batch of imgs (B x sh x sw) placed as windows inside an array of 255s; returns the
    whole destination buffer and a function that builds what it must hold from per-image results."""
    import torch
    B, sh, sw = imgs.shape
    step, dstep = sw + step_extra, dw + dstep_extra
    istride, dstride = step * sh + 7, dstep * dh + 3
    src = np.full(off + 64 + istride * B + 64, 255, np.uint8)
    base = off + 64
    for b in range(B):
        for r in range(sh):
            o = base + b * istride + r * step
            src[o:o + sw] = imgs[b, r]
    nd = off + dstride * B + 8
    d_dst = torch.full((nd,), SENT, dtype=torch.uint8, device=_dev())
    d_src = torch.from_numpy(src).to(_dev()) if on_device else None
    torch.cuda.synchronize()
    sp = (d_src.data_ptr() if on_device else src.ctypes.data) + base
    ex.remap_device(sp, B, sw, sh, step, istride, slot0, period, d_dst.data_ptr() + off, dstep, dstride,
                    src_on_device=on_device)
    torch.cuda.synchronize()

    def expect(outs):
        exp = np.full(nd, SENT, np.uint8)
        for b in range(B):
            for r in range(dh):
                o = off + b * dstride + r * dstep
                exp[o:o + dw] = outs[b][r]
        return exp
    return d_dst.cpu().numpy(), expect


SRC_SIZES = [(1, 1), (1, 9), (9, 1), (5, 3), (13, 7), (70, 6), (2, 2)]   # (sw, sh)


@pytest.mark.parametrize("maps_on_device", [False, True], ids=["host_maps", "device_maps"])
@pytest.mark.parametrize("src_on_device", [False, True], ids=["host_src", "device_src"])
def test_remap_geometries(gpu, ex, src_on_device, maps_on_device):
    import torch
    rng = np.random.default_rng(10 + 2 * src_on_device + maps_on_device)
    keep, ncase = [], 0
    for dw in range(1, 68):
        for dh in range(1, 6):
            i = ncase
            sw, sh = SRC_SIZES[i % len(SRC_SIZES)]
            B = 1 + (i % 3 == 2)
            m1, m2 = cases.random_maps(rng, dw, dh, sw, sh)
            imgs = np.stack([cases.source(rng, sh, sw, i + b) for b in range(B)])
            _set(ex, 0, m1, m2, maps_on_device, extra=(0, 5, 4, 3)[i % 4], keep=keep)
            got, expect = _run(ex, imgs, dw, dh, 0, 1, step_extra=(0, 3)[i % 2], dstep_extra=(0, 5, 2)[i % 3],
                               off=(i // 2) % 2, on_device=src_on_device)
            want = expect([ref.remap(im, m1, m2) for im in imgs])
            assert np.array_equal(got, want), (dw, dh, sw, sh, B)
            ncase += 1
            if len(keep) > 64:
                torch.cuda.synchronize()
                del keep[:]
    assert ncase == 67 * 5


def _special_cases():
    rng = np.random.default_rng(5)
    out = []
    # all 1024 table entries, on random bytes and on 0 / 255 neighbours
    for kind in (0, 1):
        out.append(("table", cases.table_maps(), cases.source(rng, 6, 8, kind)))
    ties = cases.tie_values()
    out.append(("ties", cases.grid_maps(ties, ties), cases.source(rng, 5, 5, 1)))
    out.append(("ties_random", cases.grid_maps(ties, ties), cases.source(rng, 4, 4, 0)))
    for sw, sh in ((7, 5), (1, 1), (1, 4), (6, 1)):
        for kind in (0, 1):
            out.append((f"border_{sw}x{sh}", cases.grid_maps(cases.border_values(sw), cases.border_values(sh)),
                        cases.source(rng, sh, sw, kind)))
    # a source of all 255: every inside tap counts, every outside tap must be 0
    out.append(("border_255", cases.grid_maps(cases.border_values(7), cases.border_values(5)),
                np.full((5, 7), 255, np.uint8)))
    return out


def test_remap_table_ties_borders_and_special_values(gpu, ex):
    for name, (m1, m2), img in _special_cases():
        want = ref.remap(img, m1, m2)
        if name == "table":
            ix, iy, fx, fy, _ = ref.quantise(m1, m2)
            assert len(np.unique(fy * 32 + fx)) == 1024
        if name == "border_255":
            assert (want == 0).any() and (want == 255).any() and ((want > 0) & (want < 255)).any()
        dh, dw = m1.shape
        _set(ex, 1, m1, m2)
        got, expect = _run(ex, img[None], dw, dh, 1, 1, step_extra=2, dstep_extra=1, off=1)
        assert np.array_equal(got, expect([want])), name


@pytest.mark.parametrize("ipt", [None, "1", "2", "64"], ids=["default", "ipt1", "ipt2", "ipt64"])
def test_remap_batches_and_slots(gpu, ex, monkeypatch, ipt):
    """ipt: images of a slot one thread makes from the record it holds (ORBGPU_REMAP_IPT, the
    measurement switch of tools/remap_timing.py); every setting gives the same bytes."""
    if ipt is not None:
        monkeypatch.setenv("ORBGPU_REMAP_IPT", ipt)
    rng = np.random.default_rng(6)
    dw, dh, sw, sh = 37, 9, 21, 11
    maps = [cases.random_maps(rng, dw, dh, sw, sh) for _ in range(ORB_REMAP_SLOTS)]
    for s, (m1, m2) in enumerate(maps):
        _set(ex, s, m1, m2, extra=s)
    imgs = np.stack([cases.source(rng, sh, sw, b) for b in range(5)])
    for slot0, period, B in [(0, 1, 5), (3, 1, 2), (0, 2, 5), (2, 2, 5), (1, 3, 5), (0, 4, 5), (1, 2, 1), (0, 4, 2)]:
        got, expect = _run(ex, imgs[:B], dw, dh, slot0, period, step_extra=1, dstep_extra=3)
        want = expect([ref.remap(imgs[b], *maps[slot0 + b % period]) for b in range(B)])
        assert np.array_equal(got, want), (slot0, period, B)
    # left / right differ, so a swapped slot would show
    assert not np.array_equal(ref.remap(imgs[0], *maps[0]), ref.remap(imgs[0], *maps[1]))


def test_remap_arguments(gpu, ex):
    import torch
    L = lib()
    dw, dh, sw, sh = 8, 3, 6, 4
    rng = np.random.default_rng(8)
    m1, m2 = cases.random_maps(rng, dw, dh, sw, sh)
    ex.set_remap(0, m1, m2)
    ex.set_remap(1, m1, m2)
    ex.set_remap(2, *cases.random_maps(rng, dw + 1, dh, sw, sh))     # another size
    ex.set_remap(3, None, None)                                      # unset
    src = torch.zeros(sw * sh * 2 + 8, dtype=torch.uint8, device=_dev())
    d = torch.full((dw * dh * 2 + 8,), SENT, dtype=torch.uint8, device=_dev())
    torch.cuda.synchronize()
    sp, dp = C.c_void_p(src.data_ptr()), C.c_void_p(d.data_ptr())
    call = lambda *a: L.ORBextractor_remap_batch(ex._h, *a)
    ok = (sp, 2, sw, sh, sw, sw * sh, 1, 0, 2, dp, dw, dw * dh)
    bad = [
        (None,) + ok[1:], ok[:9] + (None,) + ok[10:],                 # null pointers
        (sp, 1, sw, sh, sw, sw * sh, 1, 3, 1, dp, dw, dw * dh),       # an unset slot
        (sp, 2, sw, sh, sw, sw * sh, 1, 1, 2, dp, dw + 1, (dw + 1) * dh),   # slots of unequal size
        (sp, 2, sw, sh, sw, sw * sh, 1, 0, 0, dp, dw, dw * dh),       # slot_period < 1
        (sp, 2, sw, sh, sw, sw * sh, 1, 3, 2, dp, dw, dw * dh),       # slot0 + slot_period > slots
        (sp, 2, sw, sh, sw, sw * sh, 1, -1, 1, dp, dw, dw * dh),
        (sp, 2, sw, sh, sw - 1, sw * sh, 1, 0, 2, dp, dw, dw * dh),   # step below a row
        (sp, 2, sw, sh, sw, sw * sh, 1, 0, 2, dp, dw - 1, dw * dh),   # dst_step below a row
        (sp, 2, sw, sh, sw, sw * sh - 1, 1, 0, 2, dp, dw, dw * dh),   # overlapping sources
        (sp, 2, sw, sh, sw, sw * sh, 1, 0, 2, dp, dw, dw * dh - 1),   # overlapping destinations
        (sp, 65536, sw, sh, sw, sw * sh, 1, 0, 2, dp, dw, dw * dh),
        (sp, -1, sw, sh, sw, sw * sh, 1, 0, 2, dp, dw, dw * dh),
        (sp, 2, 0, sh, sw, sw * sh, 1, 0, 2, dp, dw, dw * dh),
        (sp, 2, sw, 16385, sw, sw * sh, 1, 0, 2, dp, dw, dw * dh),
    ]
    for a in bad:
        assert call(*a) == ORB_E_INVALID, a
    assert L.ORBextractor_remap_batch(None, *ok) == ORB_E_INVALID
    assert call(sp, 0, sw, sh, sw, sw * sh, 1, 0, 2, dp, dw, dw * dh) == 0    # an empty batch: nothing to do
    assert call(None, 0, sw, sh, sw, sw * sh, 1, 3, 1, None, dw, dw * dh) == 0
    mp = C.c_void_p(m1.ctypes.data)
    sr = lambda *a: L.ORBextractor_set_remap(ex._h, *a)
    for a in [(-1, mp, mp, dw, dh, 4 * dw, 0), (ORB_REMAP_SLOTS, mp, mp, dw, dh, 4 * dw, 0), (3, mp, None, dw, dh, 4 * dw, 0),
              (3, None, mp, dw, dh, 4 * dw, 0), (3, mp, mp, 0, dh, 4 * dw, 0), (3, mp, mp, dw, 0, 4 * dw, 0),
              (3, mp, mp, dw, 16385, 4 * dw, 0), (3, mp, mp, dw, dh, 4 * dw - 1, 0)]:
        assert sr(*a) == ORB_E_INVALID, a
    assert L.ORBextractor_set_remap(None, 0, mp, mp, dw, dh, 4 * dw, 0) == ORB_E_INVALID
    assert call(sp, 1, sw, sh, sw, sw * sh, 1, 3, 1, dp, dw, dw * dh) == ORB_E_INVALID   # slot 3 is still unset
    torch.cuda.synchronize()
    assert bool((d == SENT).all())                                   # nothing ran
    assert call(*ok) == 0
    torch.cuda.synchronize()
    want = ref.remap(np.zeros((sh, sw), np.uint8), m1, m2)
    assert np.array_equal(d.cpu().numpy()[:dw * dh].reshape(dh, dw), want)
    for s in range(ORB_REMAP_SLOTS):
        ex.set_remap(s, None, None)
    assert call(*ok) == ORB_E_INVALID                                # cleared


@pytest.mark.parametrize("maps_on_device", [False, True], ids=["host_maps", "device_maps"])
def test_set_remap_between_queued_remaps(gpu, ex, maps_on_device):
    """remap through slot 0, set_remap on slot 0 with other maps (of another size), remap again, with
    no wait between the calls: the first result follows the old maps, the second the new; many rounds,
    so that freed records would be reused while an earlier remap is still queued."""
    import torch
    rng = np.random.default_rng(9)
    sw, sh, B = 320, 200, 8
    imgs = rng.integers(0, 256, (B, sh, sw), dtype=np.uint8)
    d_src = torch.from_numpy(imgs).to(_dev())
    sizes = [(301, 190), (317, 203), (64, 64), (301, 190)]
    maps = [cases.random_maps(rng, dw, dh, sw, sh) for dw, dh in sizes]
    outs = [torch.full((B, dh, dw), SENT, dtype=torch.uint8, device=_dev()) for dw, dh in sizes]
    keep = []
    torch.cuda.synchronize()
    _set(ex, 0, *maps[0], on_device=maps_on_device, keep=keep)
    for k, (dw, dh) in enumerate(sizes):
        ex.remap_device(d_src.data_ptr(), B, sw, sh, sw, sw * sh, 0, 1, outs[k].data_ptr(), dw, dw * dh)
        if k + 1 < len(sizes):
            _set(ex, 0, *maps[k + 1], on_device=maps_on_device, keep=keep)
    torch.cuda.synchronize()
    for k in range(len(sizes)):
        got = outs[k].cpu().numpy()
        for b in (0, B - 1):
            assert np.array_equal(got[b], ref.remap(imgs[b], *maps[k])), (k, b)
    ex.set_remap(0, None, None)


# ------------------------------------------------------------------- a EuRoC stereo frame
@pytest.fixture(scope="module")
def euroc():
    scenes, _ = synthetic.sequence(31, 1, cases.W, cases.H)
    raw = np.stack([cases.render_raw(scenes[0], "left"), cases.render_raw(scenes[0], "right", shift=12.0)])
    maps = [cases.euroc_maps("left"), cases.euroc_maps("right")]
    rect = np.stack([ref.remap(raw[i], *maps[i]) for i in range(2)])
    orc = oracle_lib.OracleExtractor(1200, 1.2, 8, 20, 7)
    return dict(raw=raw, maps=maps, rect=rect, feats=[orc(r) for r in rect])


def test_euroc_stereo_pair_end_to_end(gpu, ex, euroc):
    """stereo_euroc.cc's frame input: the raw pair -> remap_batch (left / right interleaved) ->
    extract_batch on the same handle with no wait in between, everything device-resident."""
    import torch
    w, h = cases.W, cases.H
    cap = 2 * 1200 + 64
    for s in range(2):
        ex.set_remap(s, *euroc["maps"][s])
    d_raw = torch.from_numpy(euroc["raw"]).to(_dev())
    d_rect = torch.full((2, h, w), SENT, dtype=torch.uint8, device=_dev())
    d_k = torch.zeros((2, cap, 7), dtype=torch.int32, device=_dev())
    d_d = torch.zeros((2, cap, 32), dtype=torch.uint8, device=_dev())
    torch.cuda.synchronize()
    ex.remap_device(d_raw.data_ptr(), 2, w, h, w, w * h, 0, 2, d_rect.data_ptr(), w, w * h)
    n = ex.extract_device(d_rect.data_ptr(), 2, w, h, w, w * h, d_k.data_ptr(), d_d.data_ptr(), cap)   # no wait between
    torch.cuda.synchronize()
    assert np.array_equal(d_rect.cpu().numpy(), euroc["rect"])
    assert not np.array_equal(euroc["rect"][0], euroc["raw"][0])
    for b in range(2):
        ok, od = euroc["feats"][b]
        N = len(ok)
        assert N > 500 and n[b] == N
        keys = d_k[b, :N].cpu().numpy().reshape(-1).view(oracle_lib.KP_DTYPE)
        assert np.array_equal(keys.view(np.uint8), ok.view(np.uint8)) and np.array_equal(d_d[b, :N].cpu().numpy(), od)


def test_extract_rectified_is_extract_of_the_rectified(gpu, ex, euroc):
    for s in range(2):
        ex.set_remap(s, *euroc["maps"][s])
        kps, desc = ex.extract_rectified(euroc["raw"][s], slot=s)
        ok, od = euroc["feats"][s]
        assert np.array_equal(kps.view(np.uint8), ok.view(np.uint8)) and np.array_equal(desc, od)
    with pytest.raises(ValueError):
        ex.extract_rectified(euroc["raw"][0], slot=3)
