"""ctypes binding of the CPU parity oracle (oracle/liborb_oracle.so).

TEST INFRASTRUCTURE ONLY -- the checker, never the thing measured.
"""
import ctypes as C
import os
import subprocess
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
ORACLE_DIR = ROOT / "oracle"
LIB_PATH = ORACLE_DIR / "liborb_oracle.so"

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                     ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
assert KP_DTYPE.itemsize == 28


def build():
    subprocess.run(["make", "-s", "-C", str(ORACLE_DIR)], check=True)


_lib = None


def use_library(path):
    """Load another build of the same oracle sources (bench.py's -O3 -march=native timing build)."""
    global _lib, LIB_PATH
    LIB_PATH = Path(path)
    _lib = None


def lib():
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            build()
        L = C.CDLL(str(LIB_PATH))
        vp, i32, f32 = C.c_void_p, C.c_int, C.c_float
        L.ora_extractor_new.restype = vp
        L.ora_extractor_new.argtypes = [i32, f32, i32, i32, i32]
        L.ora_extractor_free.argtypes = [vp]
        L.ora_extract.argtypes = [vp, vp, i32, i32, i32, vp, vp, i32]
        L.ora_extract.restype = i32
        L.ora_extractor_level.argtypes = [vp, i32, C.POINTER(C.c_void_p), C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
        L.ora_extractor_blurred.argtypes = [vp, i32, C.POINTER(C.c_void_p), C.POINTER(i32), C.POINTER(i32)]
        L.ora_extractor_candidates.argtypes = [vp, i32, vp, i32]
        L.ora_extractor_tables.argtypes = [vp, vp, vp, vp, vp, vp, vp]
        L.ora_fastAtan2.restype = f32
        L.ora_fastAtan2.argtypes = [f32, f32]
        L.ora_sinf.restype = f32
        L.ora_sinf.argtypes = [f32]
        L.ora_cosf.restype = f32
        L.ora_cosf.argtypes = [f32]
        L.ora_fast_score.argtypes = [vp, i32]
        L.ora_descriptor_distance.argtypes = [vp, vp]
        L.ora_gaussian7_taps.argtypes = [vp]
        L.ora_resize_linear_u8.argtypes = [vp, i32, i32, i32, vp, i32, i32, i32]
        L.ora_gaussian7_u8.argtypes = [vp, i32, i32, i32, vp, i32]
        L.ora_rng_seed.argtypes = [vp, C.c_uint]
        L.ora_rng_rand.argtypes = [vp]
        L.ora_rng_random_int.argtypes = [vp, i32, i32]
        _lib = L
    return _lib


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class OracleExtractor:
    """ORBextractor(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST) restated on CPU."""

    def __init__(self, nfeatures=1200, scale_factor=1.2, nlevels=8, ini_th=20, min_th=7):
        self.L = lib()
        self.h = self.L.ora_extractor_new(nfeatures, scale_factor, nlevels, ini_th, min_th)
        assert self.h
        self.nlevels = nlevels

    def __del__(self):
        if getattr(self, "h", None):
            self.L.ora_extractor_free(self.h)
            self.h = None

    def __call__(self, img):
        img = np.ascontiguousarray(img, dtype=np.uint8)
        cap = 8192
        while True:
            kps = np.zeros(cap, KP_DTYPE)
            desc = np.zeros((cap, 32), np.uint8)
            n = self.L.ora_extract(self.h, ptr(img), img.shape[1], img.shape[0], img.strides[0],
                                   ptr(kps), ptr(desc), cap)
            if n == -1 and cap > 0:
                raise RuntimeError("oracle extraction failed (image too small?)")
            if n < 0:
                cap = -n
                continue
            return kps[:n].copy(), desc[:n].copy()

    def level(self, l):
        d, pw, ph, st = C.c_void_p(), C.c_int(), C.c_int(), C.c_int()
        assert self.L.ora_extractor_level(self.h, l, C.byref(d), C.byref(pw), C.byref(ph), C.byref(st)) == 0
        buf = (C.c_uint8 * (st.value * ph.value)).from_address(d.value)
        return np.frombuffer(buf, np.uint8).reshape(ph.value, st.value)[:, :pw.value].copy()

    def blurred(self, l):
        d, w, h = C.c_void_p(), C.c_int(), C.c_int()
        assert self.L.ora_extractor_blurred(self.h, l, C.byref(d), C.byref(w), C.byref(h)) == 0
        buf = (C.c_uint8 * (w.value * h.value)).from_address(d.value)
        return np.frombuffer(buf, np.uint8).reshape(h.value, w.value).copy()

    def candidates(self, l):
        n = self.L.ora_extractor_candidates(self.h, l, None, 0)
        out = np.zeros(max(n, 1), KP_DTYPE)
        self.L.ora_extractor_candidates(self.h, l, ptr(out), n)
        return out[:n]

    def tables(self):
        nl = self.nlevels
        sc, isc, s2, is2 = (np.zeros(nl, np.float32) for _ in range(4))
        npl = np.zeros(nl, np.int32)
        umax = np.zeros(16, np.int32)
        self.L.ora_extractor_tables(self.h, ptr(sc), ptr(isc), ptr(s2), ptr(is2), ptr(npl), ptr(umax))
        return dict(scale=sc, inv_scale=isc, sigma2=s2, inv_sigma2=is2, n_per_level=npl, umax=umax)


def oracle_stereo_matches(exL, exR, kL, dL, kR, dR, rows0, mbf, mb):
    """Frame::ComputeStereoMatches (Frame.cc:466-640) on the oracle extractors' last pyramids.
    -> (uRight, depth, kept)."""
    L = lib()
    L.ora_compute_stereo_matches.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                             C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_void_p,
                                             C.c_void_p]
    kL = np.ascontiguousarray(kL, KP_DTYPE)
    kR = np.ascontiguousarray(kR, KP_DTYPE)
    dL = np.ascontiguousarray(dL, np.uint8) if len(kL) else np.zeros((1, 32), np.uint8)
    dR = np.ascontiguousarray(dR, np.uint8) if len(kR) else np.zeros((1, 32), np.uint8)
    uR = np.zeros(max(len(kL), 1), np.float32)
    dep = np.zeros(max(len(kL), 1), np.float32)
    kept = L.ora_compute_stereo_matches(ptr(kL), ptr(dL), len(kL), ptr(kR), ptr(dR), len(kR), C.c_void_p(exL.h),
                                        C.c_void_p(exR.h), int(rows0), float(mbf), float(mb), ptr(uR), ptr(dep))
    return uR[:len(kL)], dep[:len(kL)], kept


def oracle_unproject_stereo(kps, depth, Twc, fx, fy, cx, cy):
    """Frame::UnprojectStereo (Frame.cc:666-680) for every keypoint -> (x3D N x 3, mp N);
    rows with depth <= 0 are NaN in x3D (the reference returns an empty Mat)."""
    L = lib()
    L.ora_unproject_stereo.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_float, C.c_float,
                                       C.c_float, C.c_float, C.c_void_p, C.c_void_p]
    kps = np.ascontiguousarray(kps, KP_DTYPE)
    depth = np.ascontiguousarray(depth, np.float32)
    Twc = np.ascontiguousarray(Twc, np.float32)
    n = len(kps)
    x3D = np.full((max(n, 1), 3), np.nan, np.float32)
    mp = np.zeros(max(n, 1), np.int32)
    L.ora_unproject_stereo(ptr(kps), ptr(depth), n, ptr(Twc), float(fx), float(fy), float(cx), float(cy), ptr(x3D),
                           ptr(mp))
    return x3D[:n], mp[:n]


def oracle_undistort_keypoints(keys, K, dist):
    """Frame::UndistortKeyPoints (Frame.cc:404-430) restated (oracle/stereo.c, ocv_semantics.c)."""
    L = lib()
    L.ora_undistort_keypoints.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    keys = np.ascontiguousarray(keys, KP_DTYPE)
    K = np.ascontiguousarray(K, np.float32).reshape(-1)
    dist = np.ascontiguousarray(dist, np.float32).reshape(-1)
    out = np.zeros(max(len(keys), 1), KP_DTYPE)
    L.ora_undistort_keypoints(ptr(keys), len(keys), ptr(K), ptr(dist), int(dist.size), ptr(out))
    return out[:len(keys)]


def oracle_undistort_points(pts, K, k8, has_dist=True):
    """cv::undistortPoints(pts, pts, K, D, Mat(), K) restated (OpenCV 3.2 cvUndistortPoints)."""
    L = lib()
    L.ora_undistort_points.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
    K = np.ascontiguousarray(K, np.float32).reshape(-1)
    k = np.zeros(8, np.float64)
    k[:len(k8)] = k8
    out = np.zeros_like(pts)
    L.ora_undistort_points(ptr(pts), len(pts), ptr(K), ptr(k), int(bool(has_dist)), ptr(out))
    return out


def oracle_compute_image_bounds(cols, rows, K, dist):
    L = lib()
    L.ora_compute_image_bounds.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    K = np.ascontiguousarray(K, np.float32).reshape(-1)
    dist = np.ascontiguousarray(dist, np.float32).reshape(-1)
    b = np.zeros(6, np.float32)
    L.ora_compute_image_bounds(int(cols), int(rows), ptr(K), ptr(dist), int(dist.size), ptr(b))
    return tuple(np.float32(v) for v in b)


class OracleVocabulary:
    """TemplatedVocabulary (Thirdparty/DBoW2) restated on CPU: loadFromTextFile, transform, score."""

    def __init__(self, path):
        L = lib()
        L.ora_voc_load_text.restype = C.c_void_p
        L.ora_voc_load_text.argtypes = [C.c_char_p, C.POINTER(C.c_int)]
        L.ora_voc_free.argtypes = [C.c_void_p]
        L.ora_voc_info.argtypes = [C.c_void_p] + [C.POINTER(C.c_int)] * 6
        L.ora_voc_transform_feature.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.ora_voc_transform.restype = C.c_int
        L.ora_voc_transform.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 7
        L.ora_voc_score_l1.restype = C.c_double
        L.ora_voc_score_l1.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
        self.L = L
        err = C.c_int()
        self.h = L.ora_voc_load_text(os.fsencode(str(path)), C.byref(err))
        self.err = err.value

    def __del__(self):
        if getattr(self, "h", None):
            self.L.ora_voc_free(self.h)

    def info(self):
        v = [C.c_int() for _ in range(6)]
        self.L.ora_voc_info(self.h, *[C.byref(x) for x in v])
        return dict(zip(["k", "L", "scoring", "weighting", "nodes", "words"], [x.value for x in v]))

    def transform_features(self, desc, levelsup=4):
        d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        n = len(d)
        w, wt, nd = np.zeros(n, np.uint32), np.zeros(n, np.float64), np.zeros(n, np.uint32)
        for i in range(n):
            self.L.ora_voc_transform_feature(self.h, d[i].ctypes.data, int(levelsup), w[i:].ctypes.data,
                                             wt[i:].ctypes.data, nd[i:].ctypes.data)
        return w, wt, nd

    def transform(self, desc, levelsup=4):
        """-> (words, values, fv_node, fv_start, fv_feat)."""
        d = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
        n = max(len(d), 1)
        bw, bv = np.zeros(n, np.uint32), np.zeros(n, np.float64)
        fn, fs, ff = np.zeros(n, np.uint32), np.zeros(n + 1, np.int32), np.zeros(n, np.int32)
        nb, nf = C.c_int(), C.c_int()
        self.L.ora_voc_transform(self.h, ptr(d), len(d), int(levelsup), ptr(bw), ptr(bv), C.byref(nb), ptr(fn), ptr(fs),
                                 ptr(ff), C.byref(nf))
        m = int(fs[nf.value]) if nf.value else 0
        return bw[:nb.value], bv[:nb.value], fn[:nf.value], fs[:nf.value + 1], ff[:m]

    def score(self, w1, v1, w2, v2):
        w1, w2 = np.ascontiguousarray(w1, np.uint32), np.ascontiguousarray(w2, np.uint32)
        v1, v2 = np.ascontiguousarray(v1, np.float64), np.ascontiguousarray(v2, np.float64)
        return self.L.ora_voc_score_l1(w1.ctypes.data, v1.ctypes.data, len(w1), w2.ctypes.data, v2.ctypes.data, len(w2))


# ---------------------------------------------------------------- matcher oracle
class ora_frame(C.Structure):
    _fields_ = [("N", C.c_int), ("kpsUn", C.c_void_p), ("desc", C.c_void_p), ("uRight", C.c_void_p),
                ("minX", C.c_float), ("maxX", C.c_float), ("minY", C.c_float), ("maxY", C.c_float),
                ("gridWInv", C.c_float), ("gridHInv", C.c_float), ("scaleFactors", C.c_void_p),
                ("nlevels", C.c_int), ("cellStart", C.c_void_p), ("cellIdx", C.c_void_p)]


class ora_lastframe(C.Structure):
    _fields_ = [("Tcw_cur", C.c_void_p), ("Tcw_last", C.c_void_p), ("fx", C.c_float), ("fy", C.c_float),
                ("cx", C.c_float), ("cy", C.c_float), ("mbf", C.c_float), ("mb", C.c_float),
                ("lastKeys", C.c_void_p), ("lastKeysUn", C.c_void_p), ("lastMP", C.c_void_p),
                ("lastOutlier", C.c_void_p), ("lastN", C.c_int), ("mpPos", C.c_void_p), ("mpDesc", C.c_void_p),
                ("mpObs", C.c_void_p)]


class ora_localmaps(C.Structure):
    _fields_ = [("n", C.c_int), ("inView", C.c_void_p), ("projX", C.c_void_p), ("projXR", C.c_void_p),
                ("projY", C.c_void_p), ("level", C.c_void_p), ("viewCos", C.c_void_p), ("desc", C.c_void_p),
                ("mpId", C.c_void_p)]


def _addr(a):
    return None if a is None else a.ctypes.data


class OracleFrame:
    """Frame grid (Frame.cc:230-245) over host arrays; mirrors c_orb_slam_amd.Frame fields."""

    def __init__(self, F):
        self.F = F
        self.cellStart = np.zeros(64 * 48 + 1, np.int32)
        self.cellIdx = np.zeros(max(F.N, 1), np.int32)
        s = ora_frame()
        s.N = F.N
        s.kpsUn = _addr(F.keysUn)
        s.desc = _addr(F.desc)
        s.uRight = _addr(F.uRight)
        s.minX, s.maxX, s.minY, s.maxY = F.minX, F.maxX, F.minY, F.maxY
        s.gridWInv, s.gridHInv = F.gridWInv, F.gridHInv
        s.scaleFactors = _addr(F.scale)
        s.nlevels = len(F.scale)
        s.cellStart = _addr(self.cellStart)
        s.cellIdx = _addr(self.cellIdx)
        self.s = s
        L = lib()
        L.ora_frame_build_grid.argtypes = [C.c_void_p]
        L.ora_frame_build_grid(C.byref(s))

    def features_in_area(self, x, y, r, minLevel=-1, maxLevel=-1):
        L = lib()
        L.ora_frame_features_in_area.argtypes = [C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_int, C.c_int,
                                                 C.c_void_p, C.c_int]
        out = np.zeros(max(self.F.N, 1), np.int32)
        n = L.ora_frame_features_in_area(C.byref(self.s), x, y, r, minLevel, maxLevel, ptr(out), self.F.N)
        return out[:n]


def oracle_search_last(cur, cur_mp, last, last_keys, last_mp, last_outlier, mps, th, bMono, nnratio=0.9,
                       checkOri=True):
    """SearchByProjection(Cur, Last, th, bMono) on the CPU oracle; updates cur_mp in place."""
    of = OracleFrame(cur)
    lf = ora_lastframe()
    lk = np.ascontiguousarray(last_keys, KP_DTYPE)
    lm = np.ascontiguousarray(last_mp, np.int32)
    lo = np.ascontiguousarray(last_outlier, np.uint8)
    lf.Tcw_cur, lf.Tcw_last = _addr(cur.Tcw), _addr(last.Tcw)
    lf.fx, lf.fy, lf.cx, lf.cy = cur.fx, cur.fy, cur.cx, cur.cy
    lf.mbf, lf.mb = cur.bf, cur.b
    lf.lastKeys, lf.lastKeysUn = _addr(lk), _addr(last.keysUn)
    lf.lastMP, lf.lastOutlier, lf.lastN = _addr(lm), _addr(lo), len(lm)
    lf.mpPos, lf.mpDesc, lf.mpObs = _addr(mps.pos), _addr(mps.desc), _addr(mps.obs)
    L = lib()
    L.ora_search_by_projection_last.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_float,
                                                C.c_int]
    return L.ora_search_by_projection_last(C.byref(of.s), ptr(cur_mp), C.byref(lf), th, int(bMono), nnratio,
                                           int(checkOri))


def oracle_search_local(F, cur_mp, mp_obs, in_view, proj_x, proj_xr, proj_y, level, view_cos, qdesc, mp_id, th,
                        nnratio):
    of = OracleFrame(F)
    a = [np.ascontiguousarray(in_view, np.uint8), np.ascontiguousarray(proj_x, np.float32),
         np.ascontiguousarray(proj_xr, np.float32), np.ascontiguousarray(proj_y, np.float32),
         np.ascontiguousarray(level, np.int32), np.ascontiguousarray(view_cos, np.float32),
         np.ascontiguousarray(qdesc, np.uint8), np.ascontiguousarray(mp_id, np.int32)]
    m = ora_localmaps()
    m.n = len(a[0])
    m.inView, m.projX, m.projXR, m.projY, m.level, m.viewCos, m.desc, m.mpId = [_addr(x) for x in a]
    obs = np.ascontiguousarray(mp_obs, np.int32)
    L = lib()
    L.ora_search_by_projection_local.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float,
                                                 C.c_float]
    return L.ora_search_by_projection_local(C.byref(of.s), ptr(cur_mp), ptr(obs), C.byref(m), th, nnratio)


def oracle_is_in_frustum(F, M, logScaleFactor, viewingCosLimit=0.5):
    """Frame::isInFrustum (Frame.cc:269-325) of every point of local map M (dict) in Frame F."""
    n = len(M["pos"])
    pos = np.ascontiguousarray(M["pos"], np.float32).reshape(-1, 3)
    mx, mn = np.ascontiguousarray(M["max_dist"], np.float32), np.ascontiguousarray(M["min_dist"], np.float32)
    nrm = np.ascontiguousarray(M["normal"], np.float32).reshape(-1, 3)
    skip = np.ascontiguousarray(M["skip"], np.uint8)
    r = dict(in_view=np.zeros(n, np.uint8), proj_x=np.zeros(n, np.float32), proj_xr=np.zeros(n, np.float32),
             proj_y=np.zeros(n, np.float32), level=np.zeros(n, np.int32), view_cos=np.zeros(n, np.float32))
    L = lib()
    f32 = C.c_float
    L.ora_is_in_frustum.argtypes = [C.c_void_p] + [f32] * 9 + [C.c_int, f32, C.c_int] + [C.c_void_p] * 5 + [f32] + \
        [C.c_void_p] * 6
    T = np.ascontiguousarray(F.Tcw, np.float32).reshape(16)
    nv = L.ora_is_in_frustum(ptr(T), F.fx, F.fy, F.cx, F.cy, F.bf, F.minX, F.maxX, F.minY, F.maxY, len(F.scale),
                             logScaleFactor, n, ptr(pos), ptr(mx), ptr(mn), ptr(nrm), ptr(skip), viewingCosLimit,
                             ptr(r["in_view"]), ptr(r["proj_x"]), ptr(r["proj_xr"]), ptr(r["proj_y"]), ptr(r["level"]),
                             ptr(r["view_cos"]))
    r["nvisible"] = nv
    return r


def oracle_search_local_points(F, cur_mp, M, logScaleFactor, th=1.0, nnratio=0.8):
    """Tracking::SearchLocalPoints (Tracking.cc:1143-1193) on the oracle; cur_mp updated in place."""
    fr = oracle_is_in_frustum(F, M, logScaleFactor)
    n = len(M["pos"])
    nm = 0
    if fr["nvisible"] > 0:
        nm = oracle_search_local(F, cur_mp, M["obs"], fr["in_view"], fr["proj_x"], fr["proj_xr"], fr["proj_y"],
                                 fr["level"], fr["view_cos"], np.asarray(M["desc"], np.uint8).reshape(-1, 32),
                                 np.arange(n, dtype=np.int32), th, nnratio)
    return nm, fr["nvisible"]


# ---------------------------------------------------------------- PnP oracle
def _events(fn, h):
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    buf = np.zeros(2 * 512, np.int32)
    n = fn(h, ptr(buf), 512)
    assert n <= 512, "event log overflow"
    return [(int(buf[2 * i]), int(buf[2 * i + 1])) for i in range(n)]


class OraclePnP:
    """PnPsolver(F, vpMapPointMatches) restated on CPU (reference src/PnPsolver.cc)."""

    def __init__(self, p3d, p2d, sigma2, kp_idx, n_matches, fx, fy, cx, cy):
        L = lib()
        L.ora_pnp_new.restype = C.c_void_p
        L.ora_pnp_new.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float,
                                  C.c_float, C.c_float, C.c_float]
        L.ora_pnp_free.argtypes = [C.c_void_p]
        L.ora_pnp_set_ransac.argtypes = [C.c_void_p, C.c_double, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float]
        L.ora_pnp_iterate.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p]
        for f in ("ora_pnp_iterations", "ora_pnp_max_its", "ora_pnp_min_inliers"):
            getattr(L, f).argtypes = [C.c_void_p]
        self.L = L
        self.p3d = np.ascontiguousarray(p3d, np.float32)
        self.p2d = np.ascontiguousarray(p2d, np.float32)
        self.s2 = np.ascontiguousarray(sigma2, np.float32)
        self.kp = np.ascontiguousarray(kp_idx, np.int32)
        self.n_matches = n_matches
        self.h = L.ora_pnp_new(len(self.p3d), ptr(self.p3d), ptr(self.p2d), ptr(self.s2), ptr(self.kp), n_matches,
                               fx, fy, cx, cy)

    def __del__(self):
        if getattr(self, "h", None):
            self.L.ora_pnp_free(self.h)

    def set_ransac(self, probability=0.99, minInliers=8, maxIterations=300, minSet=4, epsilon=0.4, th2=5.991):
        self.L.ora_pnp_set_ransac(self.h, probability, minInliers, maxIterations, minSet, epsilon, th2)

    def iterate(self, n_iterations, rng):
        no_more = C.c_int()
        nin = C.c_int()
        inl = np.zeros(max(self.n_matches, 1), np.uint8)
        T = np.zeros(16, np.float32)
        ok = self.L.ora_pnp_iterate(self.h, n_iterations, rng, C.byref(no_more), ptr(inl), C.byref(nin), ptr(T))
        return bool(ok), T.reshape(4, 4), inl[:self.n_matches].astype(bool), nin.value, bool(no_more.value)

    @property
    def iterations(self):
        return self.L.ora_pnp_iterations(self.h)

    def events(self):
        """The last iterate() call's events: [(hypothesis index in the call, kind)], kind 1 = best
        update, 2 = Refine failed, 3 = Refine succeeded (oracle instrumentation)."""
        return _events(self.L.ora_pnp_events, self.h)


class OracleSim3:
    """Sim3Solver(pKF1, pKF2, vpMatched12, bFixScale) restated on CPU (reference src/Sim3Solver.cc)."""

    def __init__(self, X1c, X2c, s1, s2, idx1, N1, K1, K2, bFixScale=True):
        L = lib()
        L.ora_sim3_new.restype = C.c_void_p
        L.ora_sim3_new.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                   C.c_void_p, C.c_void_p, C.c_int]
        L.ora_sim3_free.argtypes = [C.c_void_p]
        L.ora_sim3_set_ransac.argtypes = [C.c_void_p, C.c_double, C.c_int, C.c_int]
        L.ora_sim3_iterate.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p]
        L.ora_sim3_estimate.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.ora_sim3_iterations.argtypes = [C.c_void_p]
        self.L = L
        self.arrs = [np.ascontiguousarray(a, t) for a, t in
                     ((X1c, np.float32), (X2c, np.float32), (s1, np.float32), (s2, np.float32), (idx1, np.int32),
                      (K1, np.float32), (K2, np.float32))]
        X1, X2, a1, a2, ix, k1, k2 = self.arrs
        self.n_matches = N1
        self.h = L.ora_sim3_new(len(ix), ptr(X1), ptr(X2), ptr(a1), ptr(a2), ptr(ix), N1, ptr(k1), ptr(k2),
                                int(bFixScale))

    def __del__(self):
        if getattr(self, "h", None):
            self.L.ora_sim3_free(self.h)

    def set_ransac(self, probability=0.99, minInliers=6, maxIterations=300):
        self.L.ora_sim3_set_ransac(self.h, probability, minInliers, maxIterations)

    def iterate(self, n_iterations, rng):
        no_more, nin = C.c_int(), C.c_int()
        inl = np.zeros(max(self.n_matches, 1), np.uint8)
        T = np.zeros(16, np.float32)
        ok = self.L.ora_sim3_iterate(self.h, n_iterations, rng, C.byref(no_more), ptr(inl), C.byref(nin), ptr(T))
        return bool(ok), T.reshape(4, 4), inl[:self.n_matches].astype(bool), nin.value, bool(no_more.value)

    def estimate(self):
        R, t, s = np.zeros(9, np.float32), np.zeros(3, np.float32), np.zeros(1, np.float32)
        self.L.ora_sim3_estimate(self.h, ptr(R), ptr(t), ptr(s))
        return R.reshape(3, 3), t, float(s[0])

    @property
    def iterations(self):
        return self.L.ora_sim3_iterations(self.h)

    def events(self):
        """The last iterate() call's events: [(hypothesis index in the call, kind)], kind 1 = best
        update, 3 = best update returned (oracle instrumentation)."""
        return _events(self.L.ora_sim3_events, self.h)


def new_rng(seed=1):
    g = (C.c_int32 * 40)()
    lib().ora_rng_seed(g, seed)
    return g


class _BAProblem(C.Structure):
    _fields_ = [("n_kf", C.c_int), ("kf_id", C.c_void_p), ("kf_Tcw", C.c_void_p), ("kf_local", C.c_void_p),
                ("kf_cam", C.c_void_p), ("n_pt", C.c_int), ("pt_id", C.c_void_p), ("pt_pos", C.c_void_p),
                ("n_edge", C.c_int), ("edge_pt", C.c_void_p), ("edge_kf", C.c_void_p), ("edge_obs", C.c_void_p),
                ("edge_inv_sigma2", C.c_void_p)]


class _BAResult(C.Structure):
    _fields_ = [("kf_Tcw", C.c_void_p), ("pt_pos", C.c_void_p), ("edge_erase", C.c_void_p),
                ("iterations", C.c_int * 2), ("n_erased", C.c_int), ("aborted", C.c_int)]


class ba_order:
    """Context manager: run the BA / PoseOptimization oracle in the given accumulation order,
    "g2o" (the reference's sequential += order) or "canonical" (the GPU's tree order)."""

    def __init__(self, mode):
        self.mode = {"canonical": 0, "g2o": 1}[mode]

    def __enter__(self):
        L = lib()
        L.ora_ba_get_order.restype = C.c_int
        self.prev = L.ora_ba_get_order()
        L.ora_ba_set_order(self.mode)
        return self

    def __exit__(self, *a):
        lib().ora_ba_set_order(self.prev)


class _BATrace(C.Structure):
    _fields_ = [("n_solves", C.c_int), ("n_trials", C.c_int), ("solve_ini_chi2", C.c_double * 256),
                ("solve_chi2", C.c_double * 256), ("trial_chi2", C.c_double * 256),
                ("trial_lambda", C.c_double * 256)]


def oracle_local_ba(pr, stop=False):
    """Optimizer::LocalBundleAdjustment restated on CPU -> dict of outputs + LM trace."""
    return _oracle_ba(pr, stop, None)


def oracle_global_ba(pr, nIterations=10, bRobust=False, stop=False):
    """Optimizer::BundleAdjustment restated on CPU -> dict of outputs + LM trace."""
    return _oracle_ba(pr, stop, (nIterations, bRobust))


def _oracle_ba(pr, stop, glob):
    L = lib()
    L.ora_local_ba.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.ora_global_ba.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    keep = {k: np.ascontiguousarray(pr[k]) for k in ("kf_id", "kf_Tcw", "kf_local", "kf_cam", "pt_id", "pt_pos",
                                                     "edge_pt", "edge_kf", "edge_obs", "edge_inv_sigma2")}
    P = _BAProblem(len(keep["kf_id"]), ptr(keep["kf_id"]), ptr(keep["kf_Tcw"]), ptr(keep["kf_local"]),
                   ptr(keep["kf_cam"]), len(keep["pt_id"]), ptr(keep["pt_id"]), ptr(keep["pt_pos"]),
                   len(keep["edge_pt"]), ptr(keep["edge_pt"]), ptr(keep["edge_kf"]), ptr(keep["edge_obs"]),
                   ptr(keep["edge_inv_sigma2"]))
    T = np.zeros_like(keep["kf_Tcw"])
    X = np.zeros_like(keep["pt_pos"])
    er = np.zeros(len(keep["edge_pt"]), np.uint8)
    R = _BAResult(ptr(T), ptr(X), ptr(er))
    tr = _BATrace()
    st = C.c_int(1 if stop else 0)
    if glob is None:
        L.ora_local_ba(C.byref(P), C.byref(st), C.byref(R), C.byref(tr))
    else:
        L.ora_global_ba(C.byref(P), int(glob[0]), int(bool(glob[1])), C.byref(st), C.byref(R), C.byref(tr))
    return dict(kf_Tcw=T, pt_pos=X, edge_erase=er.astype(bool), iterations=tuple(R.iterations),
                n_erased=R.n_erased, aborted=bool(R.aborted),
                solve_chi2=np.array(tr.solve_chi2[:tr.n_solves]), solve_ini_chi2=np.array(tr.solve_ini_chi2[:tr.n_solves]),
                trial_chi2=np.array(tr.trial_chi2[:tr.n_trials]), trial_lambda=np.array(tr.trial_lambda[:tr.n_trials]))


# ---------------------------------------------------------------- remaining ORBmatcher searches
class ora_featvec(C.Structure):
    _fields_ = [("n_nodes", C.c_int), ("node_id", C.c_void_p), ("start", C.c_void_p), ("feat", C.c_void_p)]


def _fv(fv):
    v = ora_featvec()
    v.n_nodes = len(fv.node_id)
    v.node_id, v.start, v.feat = fv.node_id.ctypes.data, fv.start.ctypes.data, fv.feat.ctypes.data
    return v


def _u8(a):
    return np.ascontiguousarray(a, np.uint8)


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def _i32(a):
    return np.ascontiguousarray(a, np.int32)


def oracle_search_by_projection_kf(F, cur_mp, kf_mp, skip, kf_angle, mps, max_dist, min_dist, logScaleFactor, th,
                                   ORBdist, checkOri=True):
    L = lib()
    vp, i32, f32 = C.c_void_p, C.c_int, C.c_float
    L.ora_search_by_projection_kf.argtypes = [vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, f32, f32, i32, i32]
    of = OracleFrame(F)
    K = np.array([F.fx, F.fy, F.cx, F.cy], np.float32)
    kf_mp, skip, kf_angle, mx, mn = _i32(kf_mp), _u8(skip), _f32(kf_angle), _f32(max_dist), _f32(min_dist)
    return L.ora_search_by_projection_kf(C.byref(of.s), F.Tcw.ctypes.data, ptr(K), ptr(cur_mp), len(kf_mp), ptr(kf_mp),
                                         ptr(skip), ptr(kf_angle), ptr(mps.pos), ptr(mps.desc), ptr(mx), ptr(mn),
                                         float(logScaleFactor), float(th), int(ORBdist), int(bool(checkOri)))


def oracle_search_for_initialization(F1, F2, prev_matched, windowSize, nnratio=0.9, checkOri=True):
    L = lib()
    vp = C.c_void_p
    L.ora_search_for_initialization.argtypes = [vp, vp, vp, vp, C.c_int, C.c_float, C.c_int]
    o1, o2 = OracleFrame(F1), OracleFrame(F2)
    m12 = np.full(max(F1.N, 1), -1, np.int32)
    n = L.ora_search_for_initialization(C.byref(o1.s), C.byref(o2.s), ptr(prev_matched), ptr(m12), int(windowSize),
                                        float(nnratio), int(bool(checkOri)))
    return n, m12[:F1.N]


def oracle_search_by_bow_frame(kf_desc, kf_angle, kf_mp, kf_mp_bad, fvKF, f_desc, f_angle, fvF, nnratio,
                               checkOri=True):
    L = lib()
    vp, i32 = C.c_void_p, C.c_int
    L.ora_search_by_bow_frame.argtypes = [vp, vp, vp, vp, vp, i32, vp, vp, vp, i32, C.c_float, i32, vp]
    kd, fd = _u8(kf_desc).reshape(-1, 32), _u8(f_desc).reshape(-1, 32)
    out = np.full(max(len(fd), 1), -1, np.int32)
    v1, v2 = _fv(fvKF), _fv(fvF)
    km, kb, ka, fa = _i32(kf_mp), _u8(kf_mp_bad), _f32(kf_angle), _f32(f_angle)
    n = L.ora_search_by_bow_frame(C.byref(v1), ptr(km), ptr(kb), ptr(kd), ptr(ka), len(kd), C.byref(v2), ptr(fd),
                                  ptr(fa), len(fd), float(nnratio), int(bool(checkOri)), ptr(out))
    return n, out[:len(fd)]


def oracle_search_by_bow_kf(desc1, angle1, mp1, bad1, fv1, desc2, angle2, mp2, bad2, fv2, nnratio, checkOri=True):
    L = lib()
    vp, i32 = C.c_void_p, C.c_int
    L.ora_search_by_bow_kf.argtypes = [vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, i32, C.c_float, i32, vp]
    d1, d2 = _u8(desc1).reshape(-1, 32), _u8(desc2).reshape(-1, 32)
    out = np.full(max(len(d1), 1), -1, np.int32)
    a1, a2, m1, m2, b1, b2 = _f32(angle1), _f32(angle2), _i32(mp1), _i32(mp2), _u8(bad1), _u8(bad2)
    v1, v2 = _fv(fv1), _fv(fv2)
    n = L.ora_search_by_bow_kf(C.byref(v1), ptr(m1), ptr(b1), ptr(d1), ptr(a1), len(d1), C.byref(v2), ptr(m2),
                               ptr(b2), ptr(d2), ptr(a2), len(d2), float(nnratio), int(bool(checkOri)), ptr(out))
    return n, out[:len(d1)]


def oracle_search_for_triangulation(KF1, has_mp1, fv1, KF2, has_mp2, fv2, levelSigma2_2, F12, bOnlyStereo,
                                    checkOri=True):
    L = lib()
    vp, i32 = C.c_void_p, C.c_int
    L.ora_search_for_triangulation.argtypes = [vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp,
                                               vp, i32, i32, vp, i32]
    uR1 = KF1.uRight if KF1.uRight is not None else np.full(KF1.N, -1, np.float32)
    uR2 = KF2.uRight if KF2.uRight is not None else np.full(KF2.N, -1, np.float32)
    h1, h2 = _u8(has_mp1), _u8(has_mp2)
    K2 = np.array([KF2.fx, KF2.fy, KF2.cx, KF2.cy], np.float32)
    s2, F = _f32(levelSigma2_2), _f32(F12).reshape(3, 3)
    pairs = np.zeros((max(KF1.N, 1), 2), np.int32)
    v1, v2 = _fv(fv1), _fv(fv2)
    n = L.ora_search_for_triangulation(C.byref(v1), ptr(KF1.keysUn), ptr(KF1.desc), ptr(_f32(uR1)), ptr(h1), KF1.N,
                                       KF1.Tcw.ctypes.data, C.byref(v2), ptr(KF2.keysUn), ptr(KF2.desc),
                                       ptr(_f32(uR2)), ptr(h2), KF2.N, KF2.Tcw.ctypes.data, ptr(K2), ptr(KF2.scale),
                                       ptr(s2), ptr(F), int(bool(bOnlyStereo)), int(bool(checkOri)), ptr(pairs),
                                       len(pairs))
    return pairs[:n].copy()


class _PoseProblem(C.Structure):
    _fields_ = [("N", C.c_int), ("Tcw", C.c_void_p), ("has_mp", C.c_void_p), ("Xw", C.c_void_p), ("obs", C.c_void_p),
                ("inv_sigma2", C.c_void_p), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float),
                ("cy", C.c_float), ("bf", C.c_float)]


def oracle_pose_optimization(pr):
    """Optimizer::PoseOptimization restated on CPU -> dict(Tcw, outlier, inliers, trace)."""
    L = lib()
    L.ora_pose_optimization.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    a = {k: np.ascontiguousarray(pr[k], dt) for k, dt in (("Tcw", np.float32), ("has_mp", np.uint8),
                                                           ("Xw", np.float32), ("obs", np.float32),
                                                           ("inv_sigma2", np.float32))}
    N = len(a["has_mp"])
    P = _PoseProblem(N, ptr(a["Tcw"]), ptr(a["has_mp"]), ptr(a["Xw"]), ptr(a["obs"]), ptr(a["inv_sigma2"]),
                     *[float(v) for v in pr["cam"]])
    T = np.zeros(16, np.float32)
    outl = np.ascontiguousarray(pr.get("outlier", np.zeros(N, np.uint8)), np.uint8).copy()
    tr = _BATrace()
    n = L.ora_pose_optimization(C.byref(P), ptr(T), ptr(outl), C.byref(tr))
    return dict(Tcw=T.reshape(4, 4), outlier=outl, inliers=n, solve_chi2=np.array(tr.solve_chi2[:tr.n_solves]),
                solve_ini_chi2=np.array(tr.solve_ini_chi2[:tr.n_solves]),
                trial_chi2=np.array(tr.trial_chi2[:tr.n_trials]), trial_lambda=np.array(tr.trial_lambda[:tr.n_trials]))


# ---- LocalMapping / LoopClosing projection searches (oracle/matchers3.c) ----------------
def _geo_arrays(geo):
    return _f32(geo.max_dist), _f32(geo.min_dist), _f32(geo.normal if geo.normal is not None else np.zeros((1, 3)))


def oracle_search_by_projection_sim3(KF, Scw, pts, geo, skip, matched, logScaleFactor, th):
    L = lib()
    vp, i32, f32 = C.c_void_p, C.c_int, C.c_float
    L.ora_search_by_projection_sim3.argtypes = [vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, f32, i32, vp]
    of = OracleFrame(KF)
    K = np.array([KF.fx, KF.fy, KF.cx, KF.cy], np.float32)
    S = _f32(Scw).reshape(16)
    mx, mn, nrm = _geo_arrays(geo)
    m = _i32(matched).copy()
    n = L.ora_search_by_projection_sim3(C.byref(of.s), ptr(K), ptr(S), pts.n, ptr(pts.pos), ptr(pts.desc), ptr(mx),
                                        ptr(mn), ptr(nrm), ptr(_u8(skip)), float(logScaleFactor), int(th), ptr(m))
    return n, m


def oracle_fuse(KF, pts, geo, skip, logScaleFactor, th):
    L = lib()
    vp, i32, f32 = C.c_void_p, C.c_int, C.c_float
    L.ora_fuse.argtypes = [vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, f32, f32, vp]
    of = OracleFrame(KF)
    K5 = np.array([KF.fx, KF.fy, KF.cx, KF.cy, KF.bf], np.float32)
    mx, mn, nrm = _geo_arrays(geo)
    best = np.full(max(pts.n, 1), -1, np.int32)
    n = L.ora_fuse(C.byref(of.s), KF.Tcw.ctypes.data, ptr(K5), pts.n, ptr(pts.pos), ptr(pts.desc), ptr(mx), ptr(mn),
                   ptr(nrm), ptr(_u8(skip)), float(logScaleFactor), float(th), ptr(best))
    return n, best[:pts.n]


def oracle_fuse_sim3(KF, Scw, pts, geo, skip, logScaleFactor, th):
    L = lib()
    vp, i32, f32 = C.c_void_p, C.c_int, C.c_float
    L.ora_fuse_sim3.argtypes = [vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, f32, f32, vp]
    of = OracleFrame(KF)
    K = np.array([KF.fx, KF.fy, KF.cx, KF.cy], np.float32)
    S = _f32(Scw).reshape(16)
    mx, mn, nrm = _geo_arrays(geo)
    best = np.full(max(pts.n, 1), -1, np.int32)
    n = L.ora_fuse_sim3(C.byref(of.s), ptr(K), ptr(S), pts.n, ptr(pts.pos), ptr(pts.desc), ptr(mx), ptr(mn), ptr(nrm),
                        ptr(_u8(skip)), float(logScaleFactor), float(th), ptr(best))
    return n, best[:pts.n]


def oracle_search_by_sim3(KF1, mp1, KF2, mp2, pts, geo, bad, matches12, s12, R12, t12, logScaleFactor, th):
    L = lib()
    vp, f32 = C.c_void_p, C.c_float
    L.ora_search_by_sim3.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, f32, vp, vp, f32, f32]
    o1, o2 = OracleFrame(KF1), OracleFrame(KF2)
    K = np.array([KF1.fx, KF1.fy, KF1.cx, KF1.cy], np.float32)
    mx, mn, _ = _geo_arrays(geo)
    m12 = _i32(matches12).copy()
    n = L.ora_search_by_sim3(C.byref(o1.s), KF1.Tcw.ctypes.data, ptr(_i32(mp1)), C.byref(o2.s), KF2.Tcw.ctypes.data,
                             ptr(_i32(mp2)), ptr(K), ptr(pts.pos), ptr(pts.desc), ptr(mx), ptr(mn), ptr(_u8(bad)),
                             ptr(m12), float(s12), ptr(_f32(R12).reshape(9)), ptr(_f32(t12).reshape(3)),
                             float(logScaleFactor), float(th))
    return n, m12


# ---------------------------------------------------------------- Optimizer::OptimizeSim3
class ora_sim3opt_problem(C.Structure):
    _fields_ = [("N", C.c_int), ("valid", C.c_void_p), ("X1c", C.c_void_p), ("X2c", C.c_void_p),
                ("obs1", C.c_void_p), ("obs2", C.c_void_p), ("inv_sigma2_1", C.c_void_p),
                ("inv_sigma2_2", C.c_void_p), ("K1", C.c_float * 4), ("K2", C.c_float * 4), ("th2", C.c_float),
                ("bFixScale", C.c_int)]


SIM3OPT_ARRAYS = (("valid", np.uint8), ("X1c", np.float32), ("X2c", np.float32), ("obs1", np.float32),
                  ("obs2", np.float32), ("inv_sigma2_1", np.float32), ("inv_sigma2_2", np.float32))


def sim3opt_struct(pr, cls=ora_sim3opt_problem):
    """Fill a (layout-identical) problem struct; returns (struct, arrays kept alive)."""
    keep = {k: np.ascontiguousarray(pr[k], t) for k, t in SIM3OPT_ARRAYS}
    P = cls()
    P.N = int(pr["N"])
    for k, _ in SIM3OPT_ARRAYS:
        setattr(P, k, ptr(keep[k]))
    P.K1 = (C.c_float * 4)(*[float(x) for x in pr["K1"]])
    P.K2 = (C.c_float * 4)(*[float(x) for x in pr["K2"]])
    P.th2 = float(pr["th2"])
    P.bFixScale = int(pr["bFixScale"])
    return P, keep


def oracle_sim3_from_Rts(R, t, s):
    L = lib()
    L.ora_sim3_from_Rts.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_void_p]
    Rf, tf = np.ascontiguousarray(R, np.float32), np.ascontiguousarray(t, np.float32)
    S = np.zeros(8, np.float64)
    L.ora_sim3_from_Rts(ptr(Rf), ptr(tf), float(s), ptr(S))
    return S


def oracle_optimize_sim3(pr, S12):
    """Optimizer::OptimizeSim3 restated on CPU -> (nIn, S12 out, erased mask, LM trace)."""
    L = lib()
    L.ora_optimize_sim3.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.ora_optimize_sim3.restype = C.c_int
    P, keep = sim3opt_struct(pr)
    S = np.array(S12, np.float64).copy()
    er = np.zeros(max(int(pr["N"]), 1), np.uint8)
    tr = _BATrace()
    n = L.ora_optimize_sim3(C.byref(P), ptr(S), ptr(er), C.byref(tr))
    return n, S, er[:int(pr["N"])].astype(bool), dict(
        solve_chi2=np.array(tr.solve_chi2[:tr.n_solves]), trial_chi2=np.array(tr.trial_chi2[:tr.n_trials]),
        trial_lambda=np.array(tr.trial_lambda[:tr.n_trials]))


def oracle_det_exp(x):
    L = lib()
    L.ora_det_exp.argtypes = [C.c_double]
    L.ora_det_exp.restype = C.c_double
    return L.ora_det_exp(float(x))
