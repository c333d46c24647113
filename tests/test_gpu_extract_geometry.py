"""GPU ORB extraction against the CPU oracle over pyramid geometries, thresholds and the
extractor's life cycle: bit-exact padded levels, blurred levels, keypoints and descriptors.

test_gpu_extract.py runs one parameter set (1.2, 8 levels, 20 / 7) at three sizes.  The cases here
(extract_cases.py; what each one reaches is asserted on the CPU in test_extract_cases_cpu.py) are
small images whose geometry takes Extractor::setup_geometry and the kernels where those sizes never
go: single-cell levels, cells of 58 rows, union ROIs of exactly FC_MAXR, clipped last columns,
scale factors whose resize tiles need several staging rounds or fewer rows, 15 levels, nIni up to
7, thresholds of 0 and iniTh < minTh, a second image size through one extractor, ORB_E_CAPACITY,
and the geometries the device refuses.
"""
import ctypes as C

import numpy as np
import pytest

import extract_cases as ec
import oracle_lib

pytestmark = pytest.mark.gpu


def _both(gpu, case, th=(20, 7), max_batch=1):
    W, H, sf, nl, nf = case
    ex = gpu.ORBextractor(nf, sf, nl, th[0], th[1], max_width=W, max_height=H, max_batch=max_batch)
    return ex, oracle_lib.OracleExtractor(nf, sf, nl, th[0], th[1])


@pytest.mark.parametrize("case", ec.CASES, ids=ec.case_id)
def test_geometry_single_image(gpu, case):
    W, H, sf, nl, nf = case
    ex, orc = _both(gpu, case)
    img = ec.image(W, H)
    gk, gd = ex(img)
    ec.assert_extraction_equal(ex, orc, img, gk, gd, nl)
    flags, chain_from, rows = ec.extract_plan(ex)
    assert flags == 0 and chain_from == 0, (flags, chain_from)      # the default path, 16-row tiles
    assert (rows[0] <= 16).all() and (rows[1] <= 32).all() and (rows >= 1).all(), rows


@pytest.mark.parametrize("case", ec.BATCH8_CASES, ids=ec.case_id)
def test_geometry_batch_of_eight(gpu, case):
    """Eight different images in one extract_batch: the 32-row resize tile variant."""
    W, H, sf, nl, nf = case
    ex, orc = _both(gpu, case, max_batch=8)
    imgs = np.stack([ec.image(W, H, k) for k in range(8)])
    res = ex.extract_batch(imgs)
    flags, _, rows = ec.extract_plan(ex)
    assert flags == ec.PLAN_TILE32, flags
    if sf >= 2.5:
        # a full 32-row tile's source rectangle does not fit the staging budget: fewer rows
        assert 1 <= rows[1][1] < 32, rows
    else:
        assert (rows[1] == 32).all(), rows
    for b in range(8):
        ec.assert_extraction_equal(ex, orc, imgs[b], res[b][0], res[b][1], nl, index=b, what=f"image {b}:")


@pytest.mark.parametrize("case", [c for c in ec.CASES if c[:2] in ((257, 129), (330, 250))], ids=ec.case_id)
def test_geometry_dense_input(gpu, case):
    """Pure noise: every cell full (the slot capacity of tall and clipped cells), the octree
    splitting down to its feature count on every level."""
    W, H, sf, nl, nf = case
    ex, orc = _both(gpu, case)
    img = ec.noise(W, H, 11)
    gk, gd = ex(img)
    ok, _ = ec.assert_extraction_equal(ex, orc, img, gk, gd, nl)
    assert len(ok) >= nf


@pytest.mark.parametrize("kind", ["mixed", "low_contrast", "noise"])
@pytest.mark.parametrize("th", ec.THRESHOLDS, ids=lambda t: f"th{t[0]}_{t[1]}")
def test_thresholds(gpu, th, kind):
    W, H, sf, nl, nf = ec.THRESHOLD_GEOM
    ex, orc = _both(gpu, ec.THRESHOLD_GEOM, th)
    img = ec.threshold_image(kind)
    gk, gd = ex(img)
    ec.assert_extraction_equal(ex, orc, img, gk, gd, nl)
    if th == (255, 255):
        assert len(gk) == 0 and gd is None


def test_one_extractor_several_sizes(gpu):
    """A new image size makes setup_geometry free and rebuild every table and buffer."""
    nf, sf, nl = 500, 1.2, 4
    ex = gpu.ORBextractor(nf, sf, nl, 20, 7, max_width=320, max_height=240)
    orc = oracle_lib.OracleExtractor(nf, sf, nl, 20, 7)
    for k, (W, H) in enumerate([(320, 240), (200, 150), (320, 200), (320, 240)]):
        img = ec.image(W, H, k)
        gk, gd = ex(img)
        ec.assert_extraction_equal(ex, orc, img, gk, gd, nl, what=f"call {k} ({W}x{H}):")
    with pytest.raises(gpu.OrbGpuError):
        ex(ec.image(321, 240))
    img = ec.image(320, 240, 9)
    gk, gd = ex(img)
    ec.assert_extraction_equal(ex, orc, img, gk, gd, nl, what="after the refused width:")


GUARD = 64   # records after the buffer that a refused call must leave alone


def test_capacity_host_buffers(gpu):
    """ORB_E_CAPACITY: one record short is refused with the count it needs and nothing written
    past `capacity` records; the same handle then succeeds with exactly enough."""
    from c_orb_slam_amd._lib import KP_DTYPE, ORB_E_CAPACITY, lib, ptr
    W, H, sf, nl, nf = ec.THRESHOLD_GEOM
    img = ec.image(W, H)
    ok, od = oracle_lib.OracleExtractor(nf, sf, nl, 20, 7)(img)
    n_or = len(ok)
    assert n_or > 100
    ex = gpu.ORBextractor(nf, sf, nl, 20, 7, max_width=W, max_height=H)
    kps = np.zeros(n_or + GUARD, KP_DTYPE)
    desc = np.zeros((n_or + GUARD, 32), np.uint8)
    kps.view(np.uint8)[:] = 0xA5
    desc[:] = 0xA5
    n = C.c_int(-1)
    rc = lib().ORBextractor_extract(ex._h, ptr(img), W, H, W, ptr(kps), ptr(desc), n_or - 1, C.byref(n))
    assert rc == ORB_E_CAPACITY and n.value == n_or, (rc, n.value, n_or)
    assert (kps[n_or - 1:].view(np.uint8) == 0xA5).all() and (desc[n_or - 1:] == 0xA5).all()
    rc = lib().ORBextractor_extract(ex._h, ptr(img), W, H, W, ptr(kps), ptr(desc), n_or, C.byref(n))
    assert rc == 0 and n.value == n_or
    ec.assert_keypoints_equal(kps[:n_or], desc[:n_or], ok, od, nl)
    assert (kps[n_or:].view(np.uint8) == 0xA5).all() and (desc[n_or:] == 0xA5).all()


def test_capacity_device_buffers(gpu):
    """The same with keypoints and descriptors left in device memory, where the kernels write
    straight into the caller's buffers: after a call that filled them, a call with one record
    less is refused and writes no record at or past its capacity (the selected list of the
    earlier call must not be replayed into the smaller buffer)."""
    import torch
    from c_orb_slam_amd._lib import KP_DTYPE, ORB_E_CAPACITY
    W, H, sf, nl, nf = ec.THRESHOLD_GEOM
    img = ec.image(W, H)
    ok, od = oracle_lib.OracleExtractor(nf, sf, nl, 20, 7)(img)
    n_or = len(ok)
    ex = gpu.ORBextractor(nf, sf, nl, 20, 7, max_width=W, max_height=H)
    dev = torch.device("cuda", 0)
    dk = torch.full(((n_or + GUARD) * KP_DTYPE.itemsize,), 0xA5, dtype=torch.uint8, device=dev)
    dd = torch.full(((n_or + GUARD) * 32,), 0xA5, dtype=torch.uint8, device=dev)
    n = ex.extract_host_to_device(img, dk.data_ptr(), dd.data_ptr(), n_or)
    assert n[0] == n_or
    hk = dk.cpu().numpy()
    hd = dd.cpu().numpy().reshape(-1, 32)
    ec.assert_keypoints_equal(hk[:n_or * KP_DTYPE.itemsize].view(KP_DTYPE), hd[:n_or], ok, od, nl)
    assert (hk[n_or * KP_DTYPE.itemsize:] == 0xA5).all() and (hd[n_or:] == 0xA5).all()
    dk.fill_(0xA5)
    dd.fill_(0xA5)
    torch.cuda.synchronize()
    with pytest.raises(gpu.OrbGpuError) as e:
        ex.extract_host_to_device(img, dk.data_ptr(), dd.data_ptr(), n_or - 1)
    assert e.value.code == ORB_E_CAPACITY
    hk = dk.cpu().numpy()
    hd = dd.cpu().numpy().reshape(-1, 32)
    assert (hk[(n_or - 1) * KP_DTYPE.itemsize:] == 0xA5).all() and (hd[n_or - 1:] == 0xA5).all()


@pytest.mark.parametrize("case", ec.REJECTED, ids=ec.case_id)
def test_rejected_geometry_then_valid_image(gpu, case):
    """A level without a cell row (the reference divides by zero) and a portrait image (the octree
    has no initial node) are refused; the same handle then extracts a valid size, and a size it
    extracted before, correctly."""
    W, H, sf, nl, nf = case
    ex = gpu.ORBextractor(nf, sf, nl, 20, 7, max_width=240, max_height=240)
    orc = oracle_lib.OracleExtractor(nf, sf, nl, 20, 7)
    for k in range(2):
        img = ec.image(240, 180, k)
        gk, gd = ex(img)
        ec.assert_extraction_equal(ex, orc, img, gk, gd, nl, what=f"round {k}:")
        with pytest.raises(gpu.OrbGpuError):
            ex(ec.image(W, H))
        with pytest.raises(gpu.OrbGpuError):   # no level of the refused call is on offer
            ex.image_pyramid_level(0)
    img = ec.image(200, 150)
    gk, gd = ex(img)
    ec.assert_extraction_equal(ex, orc, img, gk, gd, nl, what="new size:")
    # a handle whose first call is the refused one
    ex2 = gpu.ORBextractor(nf, sf, nl, 20, 7, max_width=240, max_height=240)
    with pytest.raises(gpu.OrbGpuError):
        ex2(ec.image(W, H))
    gk, gd = ex2(img)
    ec.assert_extraction_equal(ex2, orc, img, gk, gd, nl, what="fresh handle:")


def test_rejected_parameters(gpu):
    with pytest.raises(gpu.OrbGpuError):
        gpu.ORBextractor(500, 1.2, 16, 20, 7, max_width=320, max_height=240)
    with pytest.raises(gpu.OrbGpuError):
        gpu.ORBextractor(500, 1.0, 4, 20, 7, max_width=320, max_height=240)
    # nFeaturesPerLevel + 8 beyond the device octree's node pool: the oracle runs it, the device
    # refuses it
    img = ec.noise(320, 240, 1)
    assert len(oracle_lib.OracleExtractor(2000, 1.2, 1, 20, 7)(img)[0]) >= 2000
    ex = gpu.ORBextractor(2000, 1.2, 1, 20, 7, max_width=320, max_height=240)
    for _ in range(2):
        with pytest.raises(gpu.OrbGpuError):
            ex(img)
    with pytest.raises(gpu.OrbGpuError):   # one feature beyond the pool: 633 + 8 > 640
        gpu.ORBextractor(633, 1.2, 1, 20, 7, max_width=320, max_height=240)(img)
    # a new handle that fills the pool exactly (632 + 8 = kOctNMax) works on the same image
    ex2, orc = _both(gpu, (320, 240, 1.2, 1, 632))
    gk, gd = ex2(img)
    ok, _ = ec.assert_extraction_equal(ex2, orc, img, gk, gd, 1)
    assert len(ok) >= 632
