"""The RGB-D sensor path on the GPU vs its numpy restatement (tests/rgbd_ref.py), byte for byte:

* ORBextractor_cvtColor_batch -- the cvtColor of Tracking::GrabImageStereo / GrabImageRGBD /
  GrabImageMonocular: widths around the 4-pixel quad and the 64-lane wave, 3 and 4 channels, both
  byte orders, padded row strides on both sides, a destination one byte off its allocation, batches,
  host and device sources; sentinel bytes show that nothing outside `width` is written;
* Frame_ComputeStereoFromRGBD[_batch] -- Frame::ComputeStereoFromRGBD with GrabImageRGBD's depth
  conversion: host form over N, depth type, factor and row stride; device batch over more frames
  than one launch carries, plain and deferred; invalid arguments;
* a TUM-shaped RGB-D frame end to end (SURVEY config 1's RGB-D sibling): cvtColor -> extraction ->
  UndistortKeyPoints -> ComputeStereoFromRGBD -> MapPoint_CreateStereo, device-resident throughout.

Both stages are exactly specified, so every comparison is np.array_equal on bytes.  cv::cvtColor is
"parity unpinned" (OpenCV absent); its restatement is pinned on CPU by tests/test_rgbd_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib
import rgbd_cases as cases
import rgbd_ref as ref
from c_orb_slam_amd import synthetic
from c_orb_slam_amd._lib import ORB_E_INVALID, lib, orb_newpoints, orb_rgbd
from undistort_cases import CAMERAS, K_of

pytestmark = pytest.mark.gpu

SENT = 0xCD
PER_LAUNCH = 44   # frame_input.hpp kRgbdPerLaunch


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bytes(a), _bytes(b))


@pytest.fixture(scope="module")
def ex(gpu):
    return gpu.ORBextractor(1000, 1.2, 8, 20, 7, max_width=640, max_height=480, max_batch=3)


@pytest.fixture(scope="module")
def matcher(gpu):
    return gpu.ORBmatcher(0.9, True)


# ------------------------------------------------------------------------------ cvtColor
@pytest.mark.parametrize("on_device", [False, True], ids=["host_src", "device_src"])
@pytest.mark.parametrize("ch", [3, 4])
def test_cvtcolor_geometries(gpu, ex, ch, on_device):
    import torch
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(100 * ch + on_device)
    kinds = ["random", "primaries", "ramp"]
    ncase = 0
    for w in (1, 3, 4, 5, 63, 64, 67):
        for h in (1, 5):
            for B in (1, 5):
                imgs = np.stack([cases.color_image(rng, h, w, ch, kinds[(b + w) % 3]) for b in range(B)])
                for rgb in (True, False):
                    want = ref.cvt_gray(imgs, rgb)
                    for step in (w * ch, w * ch + 5):
                        for gstep in (w, w + 3):
                            for off in (0, 1):   # first byte of both buffers inside their allocations
                                istride, gstride = step * h + 7, gstep * h + 3
                                src = rng.integers(0, 256, off + istride * B + 8, dtype=np.uint8)
                                exp = np.full(off + gstride * B + 8, SENT, np.uint8)
                                for b in range(B):
                                    for r in range(h):
                                        o = off + b * istride + r * step
                                        src[o:o + w * ch] = imgs[b, r].reshape(-1)
                                        o = off + b * gstride + r * gstep
                                        exp[o:o + w] = want[b, r]
                                d_gray = torch.full((len(exp),), SENT, dtype=torch.uint8, device=dev)
                                d_src = torch.from_numpy(src).to(dev) if on_device else None
                                torch.cuda.synchronize()
                                sp = d_src.data_ptr() if on_device else src.ctypes.data
                                ex.cvtColor_device(sp + off, B, w, h, ch, rgb, step, istride, d_gray.data_ptr() + off,
                                                   gstep, gstride, src_on_device=on_device)
                                torch.cuda.synchronize()
                                got = d_gray.cpu().numpy()
                                assert np.array_equal(got, exp), (w, h, B, rgb, step, gstep, off)
                                ncase += 1
    assert ncase == 7 * 2 * 2 * 2 * 2 * 2 * 2


def test_cvtcolor_arguments(gpu, ex):
    import torch
    dev = torch.device("cuda", 0)
    L = lib()
    w, h = 8, 3
    src = torch.zeros(w * h * 4, dtype=torch.uint8, device=dev)
    g = torch.full((w * h + 8,), SENT, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    call = lambda *a: L.ORBextractor_cvtColor_batch(ex._h, *a)
    sp, gp = C.c_void_p(src.data_ptr()), C.c_void_p(g.data_ptr())
    assert call(sp, 1, w, h, 1, 1, w, w * h, 1, gp, w, w * h) == ORB_E_INVALID      # the reference makes no call
    assert call(sp, 1, w, h, 2, 1, 2 * w, 2 * w * h, 1, gp, w, w * h) == ORB_E_INVALID
    assert call(sp, 1, w, h, 3, 1, 3 * w - 1, 3 * w * h, 1, gp, w, w * h) == ORB_E_INVALID   # step < a row
    assert call(sp, 1, w, h, 3, 1, 3 * w, 3 * w * h, 1, gp, w - 1, w * h) == ORB_E_INVALID   # gray_step < width
    assert call(None, 1, w, h, 3, 1, 3 * w, 3 * w * h, 1, gp, w, w * h) == ORB_E_INVALID
    assert call(sp, 1, w, h, 3, 1, 3 * w, 3 * w * h, 1, None, w, w * h) == ORB_E_INVALID
    assert call(sp, -1, w, h, 3, 1, 3 * w, 3 * w * h, 1, gp, w, w * h) == ORB_E_INVALID
    assert L.ORBextractor_cvtColor_batch(None, sp, 1, w, h, 3, 1, 3 * w, 3 * w * h, 1, gp, w, w * h) == ORB_E_INVALID
    for b_, w_, h_ in [(0, w, h), (1, 0, h), (1, w, 0)]:                             # empty: nothing to do
        assert call(sp, b_, w_, h_, 3, 1, 3 * w, 3 * w * h, 1, gp, w, w * h) == 0
    torch.cuda.synchronize()
    assert bool((g == SENT).all())


# ------------------------------------------------------------------- ComputeStereoFromRGBD
@pytest.fixture(scope="module")
def maps():
    rng = np.random.default_rng(77)
    return {np.uint16: cases.depth_u16(rng, 48, 64), np.float32: cases.depth_f32(rng, 48, 64)}


@pytest.mark.parametrize("extra", [0, 6], ids=["tight", "pitch+6"])
@pytest.mark.parametrize("dtype", [np.uint16, np.float32], ids=["u16", "f32"])
def test_stereo_from_rgbd_host(gpu, matcher, maps, dtype, extra):
    depth = cases.in_pitch(maps[dtype], extra)
    assert depth.strides[0] == 64 * depth.itemsize + extra
    for N in (0, 1, 63, 64, 65, 1000):
        keys, keysUn = cases.keypoints(np.random.default_rng(N), N, 64, 48)
        for factor in cases.FACTORS:
            uR, dep, n = matcher.ComputeStereoFromRGBD(keys, keysUn, depth, factor, 40.0)
            eu, ed, en = ref.stereo_from_rgbd(keys, keysUn, maps[dtype], factor, 40.0)
            assert _same(dep, ed), (N, factor)
            assert _same(uR, eu), (N, factor)
            assert n == en, (N, factor, n, en)
            if N >= 63:   # every special row is in: the four inside ones have a pixel, the rest none
                ins, outs = cases.special_points(64, 48)
                assert np.all(dep[len(ins):len(ins) + len(outs)] == -1)
                assert (dep == -1).any() and (dep > 0).any()


def _device_frames(rng, nframes, dev, sentinel=-7.0):
    import torch
    sizes = [(64, 48), (37, 29), (101, 7)]
    pool = {}
    for i, (w, h) in enumerate(sizes):
        for dt, mk in ((np.uint16, cases.depth_u16), (np.float32, cases.depth_f32)):
            m = mk(rng, h, w)
            pool[(i, dt)] = (m, torch.from_numpy(m).to(dev))
    frames, expect = [], []
    for f in range(nframes):
        N = [0, 5, 300, 65, 1000, 0, 64][f % 7]
        i, dt = f % 3, (np.uint16, np.float32)[(f // 3) % 2]
        m, d_m = pool[(i, dt)]
        w, h = sizes[i]
        keys, keysUn = cases.keypoints(rng, N, w, h)
        factor = cases.FACTORS[f % 4]
        mbf = 40.0 + f
        t = lambda k: torch.from_numpy(k.view(np.int32).reshape(len(k), 7).copy()).to(dev)
        frames.append(dict(keys=t(keys), keysUn=t(keysUn), depth=d_m, depthMapFactor=factor, mbf=mbf,
                           uRight=torch.full((N + 2,), sentinel, device=dev),
                           depth_out=torch.full((N + 2,), sentinel, device=dev)))
        expect.append(ref.stereo_from_rgbd(keys, keysUn, m, factor, mbf))
    return frames, expect


def _check_frames(frames, expect, nd, sentinel=-7.0):
    for f, (F, (eu, ed, en)) in enumerate(zip(frames, expect)):
        N = len(eu)
        u, d = F["uRight"].cpu().numpy(), F["depth_out"].cpu().numpy()
        assert _same(u[:N], eu) and _same(d[:N], ed), f
        assert np.all(u[N:] == sentinel) and np.all(d[N:] == sentinel), f   # nothing past N
        assert nd[f] == en, (f, nd[f], en)


def test_stereo_from_rgbd_device_batch(gpu, matcher):
    """PER_LAUNCH + 1 frames (two launches) mixing N = 0 frames, both depth types and three image
    sizes; the deferred form gives the same bytes and its counts only at ORBmatcher_finish."""
    import torch
    dev = torch.device("cuda", 0)
    nframes = PER_LAUNCH + 1
    frames, expect = _device_frames(np.random.default_rng(9), nframes, dev)
    assert sum(e[2] for e in expect) > 0 and any(len(e[0]) == 0 for e in expect)
    torch.cuda.synchronize()
    nd = matcher.ComputeStereoFromRGBD_device(frames)
    torch.cuda.synchronize()
    _check_frames(frames, expect, nd)
    # deferred: queued, the counts untouched until the chain is finished
    frames2, expect2 = _device_frames(np.random.default_rng(9), nframes, dev)
    torch.cuda.synchronize()
    nd2, finish = matcher.ComputeStereoFromRGBD_device(frames2, deferred=True)
    assert np.all(nd2 == 0)
    finish()
    torch.cuda.synchronize()
    _check_frames(frames2, expect2, nd2)
    for a, b in zip(frames, frames2):
        assert _same(a["uRight"].cpu().numpy(), b["uRight"].cpu().numpy())
        assert _same(a["depth_out"].cpu().numpy(), b["depth_out"].cpu().numpy())
    # the matcher is back in host mode
    keys, keysUn = cases.keypoints(np.random.default_rng(1), 10, 64, 48)
    m = cases.depth_u16(np.random.default_rng(2), 48, 64)
    uR, dep, n = matcher.ComputeStereoFromRGBD(keys, keysUn, m, 1.0, 40.0)
    eu, ed, en = ref.stereo_from_rgbd(keys, keysUn, m, 1.0, 40.0)
    assert _same(uR, eu) and _same(dep, ed) and n == en


def test_stereo_from_rgbd_invalid_arguments(gpu, matcher):
    L = lib()
    N = 16
    keys, keysUn = cases.keypoints(np.random.default_rng(4), N, 64, 48)
    depth = cases.depth_u16(np.random.default_rng(5), 48, 64)
    uR, dep = np.full(N, -7, np.float32), np.full(N, -7, np.float32)
    nd = np.full(1, -7, np.int32)

    def q(**kw):
        a = dict(N=N, keys=keys.ctypes.data, keysUn=keysUn.ctypes.data, depth=depth.ctypes.data, depth_type=0,
                 cols=64, rows=48, step=128, depthMapFactor=1.0, mbf=40.0, uRight=uR.ctypes.data,
                 depth_out=dep.ctypes.data)
        a.update(kw)
        return orb_rgbd(**a)

    bad = [q(N=-1), q(keys=None), q(keysUn=None), q(depth=None), q(uRight=None), q(depth_out=None),
           q(depth_type=2), q(depth_type=-1), q(step=127), q(depth_type=1, step=255), q(cols=-1)]
    for b in bad:
        assert L.Frame_ComputeStereoFromRGBD(matcher._h, C.byref(b), nd.ctypes.data_as(C.c_void_p)) == ORB_E_INVALID
        two = (orb_rgbd * 2)(q(), b)   # one bad frame refuses the whole batch before anything runs
        nd2 = np.full(2, -7, np.int32)
        assert L.Frame_ComputeStereoFromRGBD_batch(matcher._h, 2, two, nd2.ctypes.data_as(C.c_void_p)) == ORB_E_INVALID
        assert np.all(nd2 == -7)
    assert L.Frame_ComputeStereoFromRGBD_batch(matcher._h, -1, None, None) == ORB_E_INVALID
    assert L.Frame_ComputeStereoFromRGBD_batch(matcher._h, 1, None, None) == ORB_E_INVALID
    assert L.Frame_ComputeStereoFromRGBD(matcher._h, None, None) == ORB_E_INVALID
    assert np.all(uR == -7) and np.all(dep == -7) and nd[0] == -7
    # a valid call on the same arrays, ndepth omitted
    assert L.Frame_ComputeStereoFromRGBD(matcher._h, C.byref(q()), None) == 0
    eu, ed, _ = ref.stereo_from_rgbd(keys, keysUn, depth, 1.0, 40.0)
    assert _same(uR, eu) and _same(dep, ed)
    assert L.Frame_ComputeStereoFromRGBD_batch(matcher._h, 0, None, None) == 0


# ------------------------------------------------------------------- a TUM RGB-D frame
@pytest.fixture(scope="module")
def tum():
    cam, d, w, h = CAMERAS["tum1"]
    grays, _ = synthetic.sequence(5, 3, w, h)
    rng = np.random.default_rng(21)
    color = np.stack([cases.spread_gray(rng, g) for g in grays])
    gray = ref.cvt_gray(color, True)
    orc = oracle_lib.OracleExtractor(1000, 1.2, 8, 20, 7)
    feats = [orc(g) for g in gray]
    depth = cases.depth_u16(rng, h, w, holes=0.2)
    return dict(cam=cam, dist=np.float32(d), w=w, h=h, color=color, gray=gray, feats=feats, depth=depth)


def test_tum_rgbd_frame_end_to_end(gpu, ex, matcher, tum):
    """Frame(imGray, imDepth, ...) of Tracking::GrabImageRGBD and the new map points of
    StereoInitialization, device-resident: TUM fr1 camera, 640x480, 1,000 features, bf 40,
    DepthMapFactor 5000.  Every stage equals its reference bit for bit."""
    import torch
    dev = torch.device("cuda", 0)
    cam, dist, w, h = tum["cam"], tum["dist"], tum["w"], tum["h"]
    fx, fy, cx, cy = cam
    B, cap, bf = 3, 2 * 1000 + 64, 40.0
    d_col = torch.from_numpy(tum["color"]).to(dev)
    d_gray = torch.zeros((B, h, w), dtype=torch.uint8, device=dev)
    d_k = torch.zeros((B, cap, 7), dtype=torch.int32, device=dev)
    d_d = torch.zeros((B, cap, 32), dtype=torch.uint8, device=dev)
    d_u = torch.zeros_like(d_k)
    d_depth = torch.from_numpy(tum["depth"]).to(dev)
    d_uR = torch.full((B, cap), -7.0, device=dev)
    d_z = torch.full((B, cap), -7.0, device=dev)
    Twc = np.eye(4, dtype=np.float32)
    Twc[:3, 3] = (0.3, -0.2, 1.5)
    d_T = torch.from_numpy(Twc.reshape(16)).to(dev)
    scale = ex.GetScaleFactors()
    d_s = torch.from_numpy(scale).to(dev)
    d_X = torch.zeros((B, cap, 3), device=dev)
    d_row = torch.full((B, cap), -7, dtype=torch.int32, device=dev)
    d_nrm, d_mx, d_mn = torch.zeros((B, cap, 3), device=dev), torch.zeros((B, cap), device=dev), torch.zeros(
        (B, cap), device=dev)
    torch.cuda.synchronize()
    ex.cvtColor_device(d_col.data_ptr(), B, w, h, 3, True, 3 * w, 3 * w * h, d_gray.data_ptr(), w, w * h)
    n = ex.extract_device(d_gray.data_ptr(), B, w, h, w, w * h, d_k.data_ptr(), d_d.data_ptr(), cap)   # no wait between
    matcher.UndistortKeyPoints_device([dict(keys=d_k[b, :n[b]], keysUn=d_u[b, :n[b]], K=K_of(cam), dist=dist)
                                       for b in range(B)])
    nd = matcher.ComputeStereoFromRGBD_device(
        [dict(keys=d_k[b, :n[b]], keysUn=d_u[b, :n[b]], depth=d_depth, depthMapFactor=cases.TUM_FACTOR, mbf=bf,
              uRight=d_uR[b, :n[b]], depth_out=d_z[b, :n[b]]) for b in range(B)])
    qs = [orb_newpoints(int(n[b]), d_u[b].data_ptr(), d_z[b].data_ptr(), d_T.data_ptr(), fx, fy, cx, cy,
                        d_s.data_ptr(), len(scale), 1000 * b, d_X[b].data_ptr(), d_row[b].data_ptr(),
                        d_nrm[b].data_ptr(), d_mx[b].data_ptr(), d_mn[b].data_ptr()) for b in range(B)]
    assert lib().MapPoint_CreateStereo_batch_device(matcher._h, B, (orb_newpoints * B)(*qs)) == 0
    torch.cuda.synchronize()
    assert np.array_equal(d_gray.cpu().numpy(), tum["gray"])
    for b in range(B):
        ok, od = tum["feats"][b]
        N = len(ok)
        assert n[b] == N
        keys = d_k[b, :N].cpu().numpy().reshape(-1).view(oracle_lib.KP_DTYPE)
        assert _same(keys, ok) and np.array_equal(d_d[b, :N].cpu().numpy(), od)
        oku = oracle_lib.oracle_undistort_keypoints(ok, K_of(cam), dist)
        assert _same(d_u[b, :N].cpu().numpy().reshape(-1).view(oracle_lib.KP_DTYPE), oku)
        eu, ed, en = ref.stereo_from_rgbd(ok, oku, tum["depth"], cases.TUM_FACTOR, bf)
        assert en > 500                       # Tracking::StereoInitialization's test, by the reference alone
        assert (ed == -1).any()
        assert nd[b] == en
        assert _same(d_uR[b, :N].cpu().numpy(), eu) and _same(d_z[b, :N].cpu().numpy(), ed)
        assert bool((d_uR[b, N:] == -7).all()) and bool((d_z[b, N:] == -7).all())
        x3, _ = oracle_lib.oracle_unproject_stereo(oku, ed, Twc, fx, fy, cx, cy)
        has = ed > 0
        assert np.array_equal(d_X[b, :N].cpu().numpy()[has], x3[has])
        assert np.array_equal(d_row[b, :N].cpu().numpy(), np.where(has, 1000 * b + np.arange(N), -1))


@pytest.mark.parametrize("ch", [3, 4])
def test_extract_color_is_extract_of_the_grey(gpu, ex, tum, ch):
    """ORBextractor.extract_color (host colour image in, host features out) equals operator() on
    the reference grey; BGR(A) input with rgb=False gives the same."""
    col = tum["color"][0]
    if ch == 4:
        col = np.concatenate([col, np.full(col.shape[:2] + (1,), 200, np.uint8)], axis=2)
    ok, od = tum["feats"][0]
    for rgb, img in ((True, col), (False, np.ascontiguousarray(col[..., [2, 1, 0] + ([3] if ch == 4 else [])]))):
        kps, desc = ex.extract_color(img, rgb)
        assert _same(kps, ok) and np.array_equal(desc, od)
