"""Seeded SearchByProjection problems.

frame_pair / local_queries build them from real extractor output: frame t+1 is frame t seen by a
rotated camera (synthetic.sequence), so the map points lifted from frame t's keypoints project onto
frame t+1 through K R K^-1; the matchers then search the windows of Tracking's calls
(Tracking.cc:869-892 th 7/15, 1184-1191 th 1/3/5).

synth_pair / synth_local / synth_local_map build them from numpy alone, at any keypoint count,
image size and bounds, with the ingredients that make the greedy search ambiguous (descriptor
prototypes, duplicated map points, one crowded grid cell, keypoints on and outside the bounds).
PAIR_CASES and the functions after it are the shape matrix of tests/test_gpu_match_shapes.py;
tests/test_match_cases_cpu.py asserts on the oracle alone that the matrix is not vacuous.
"""
import functools
from collections import namedtuple

import numpy as np

from c_orb_slam_amd import synthetic
from c_orb_slam_amd._lib import KP_DTYPE
from c_orb_slam_amd.orb import Frame, MapPoints


def frame_pair(kps0, desc0, kps1, desc1, R, K4, w, h, scale, rng, stereo=False, bf=synthetic.KITTI_BF,
               mp_fraction=0.9, obs_zero_fraction=0.1, outlier_fraction=0.03):
    fx, fy, cx, cy = K4
    uR1 = None
    if stereo:
        d1 = rng.uniform(5, 50, size=len(kps1)).astype(np.float32)
        uR1 = np.where(rng.random(len(kps1)) < 0.6, kps1["x"] - np.float32(bf) / d1, -1).astype(np.float32)
    last = Frame(kps0, desc0, scale, np.eye(4, dtype=np.float32), fx, fy, cx, cy, bf if stereo else 0.0, w, h)
    cur = Frame(kps1, desc1, scale, synthetic.pose_from_rotation(R), fx, fy, cx, cy, bf if stereo else 0.0, w, h,
                uRight=uR1)
    X = synthetic.lift_map_points(rng, kps0, K4)
    n0 = len(kps0)
    mps = MapPoints(X, desc0, np.where(rng.random(n0) < obs_zero_fraction, 0, rng.integers(1, 6, n0)))
    last_mp = np.where(rng.random(n0) < mp_fraction, np.arange(n0), -1).astype(np.int32)
    last_outlier = (rng.random(n0) < outlier_fraction).astype(np.uint8)
    return cur, last, mps, last_mp, last_outlier


def local_queries(kps0, desc0, H, rng, nlevels=8):
    """isInFrustum outputs for map points lifted from kps0: projections through H."""
    n = len(kps0)
    p = np.stack([kps0["x"], kps0["y"], np.ones(n, np.float32)], 1).astype(np.float64) @ H.T
    px = (p[:, 0] / p[:, 2]).astype(np.float32)
    py = (p[:, 1] / p[:, 2]).astype(np.float32)
    pxr = (px - rng.uniform(1, 60, n)).astype(np.float32)
    level = np.clip(kps0["octave"] + rng.integers(-1, 2, n), 0, nlevels - 1).astype(np.int32)
    view_cos = rng.uniform(0.99, 1.0, n).astype(np.float32)
    in_view = (rng.random(n) < 0.95).astype(np.uint8)
    return in_view, px, pxr, py, level, view_cos


def local_map(rng, kps, desc, scale, Twc=np.eye(4, dtype=np.float32), extra=300, K4=None):
    """Map points lifted from a keyframe's keypoints (world = that frame's camera, then Twc), with
    the MapPoint fields UpdateNormalAndDepth sets (MapPoint.cc:349-371), plus points that fail
    each isInFrustum test."""
    fx, fy, cx, cy = K4 if K4 is not None else synthetic.intrinsics(synthetic.KITTI_W, synthetic.KITTI_H)
    n = len(kps)
    d = rng.uniform(4.0, 60.0, n)
    Xc = np.stack([(kps["x"] - cx) / fx * d, (kps["y"] - cy) / fy * d, d], 1)
    oct_ = kps["octave"].astype(int)
    # extras: behind the camera, far outside the image, scale-invariance misses, oblique normals
    e = rng.integers(0, 4, extra)
    Xe = rng.normal(0, 1, (extra, 3)) * [10, 5, 20]
    Xe[e == 0, 2] = -np.abs(Xe[e == 0, 2]) - 1
    Xe[e == 1, :2] *= 50
    Xe[e >= 2, 2] = np.abs(Xe[e >= 2, 2]) + 5
    X = np.vstack([Xc, Xe])
    oct_all = np.concatenate([oct_, rng.integers(0, 8, extra)])
    dist = np.linalg.norm(X, axis=1)
    mx = dist * scale[oct_all]
    mx[n:][e[:] == 2] *= rng.choice([0.3, 3.0], int((e == 2).sum()))      # outside [0.8 min, 1.2 max]
    mn = mx / scale[7]
    nrm = X / dist[:, None]
    tilt = np.where(np.concatenate([rng.random(n) < 0.05, e == 3]), 1.5, 0.1)
    nrm = nrm + rng.normal(0, 1, nrm.shape) * tilt[:, None]
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    R, t = Twc[:3, :3].astype(np.float64), Twc[:3, 3].astype(np.float64)
    Xw = X @ R.T + t
    nw = nrm @ R.T
    m = len(Xw)
    dsc = np.vstack([desc, rng.integers(0, 256, (extra, 32), dtype=np.uint8)])
    return dict(pos=Xw.astype(np.float32), desc=dsc, obs=rng.integers(0, 5, m).astype(np.int32),
                max_dist=mx.astype(np.float32), min_dist=mn.astype(np.float32), normal=nw.astype(np.float32),
                skip=(rng.random(m) < 0.08).astype(np.uint8))


# ------------------------------------------------------------------ numpy-only problems
GRID_COLS, GRID_ROWS = 64, 48
WIDE_BOUNDS = (-31.5, 1270.25, -12.75, 390.5)   # ComputeImageBounds of a distorted 1241 x 376 camera


def scale_factors(nlevels=8, factor=1.2):
    """mvScaleFactor as the extractor accumulates it in float."""
    s = np.ones(nlevels, np.float32)
    for i in range(1, nlevels):
        s[i] = s[i - 1] * np.float32(factor)
    return s


def _flip_bits(rng, d, k):
    """Flip up to k[i] random bits of descriptor row i, in place."""
    for nb in range(1, int(k.max(initial=0)) + 1):
        rows = np.nonzero(k >= nb)[0]
        bit = rng.integers(0, 256, len(rows))
        d[rows, bit >> 3] ^= (1 << (bit & 7)).astype(np.uint8)


def _descriptors(rng, n, protos):
    if protos is None:
        return rng.integers(0, 256, (n, 32), dtype=np.uint8)
    d = protos[rng.integers(0, len(protos), n)].copy()
    _flip_bits(rng, d, rng.integers(0, 9, n))
    return d


def _keys(n):
    k = np.zeros(n, KP_DTYPE)
    k["size"] = 31.0
    return k


def _project(T, K4, X):
    """Pinhole projection of world points through a 4 x 4 pose, in double."""
    fx, fy, cx, cy = K4
    Xc = X.astype(np.float64) @ T[:3, :3].astype(np.float64).T + T[:3, 3].astype(np.float64)
    z = Xc[:, 2]
    return fx * Xc[:, 0] / z + cx, fy * Xc[:, 1] / z + cy, z


def synth_pair(rng, n_last, n_cur, w, h, *, bounds=None, stereo=False, pool=0, dup_frac=0.0, cluster_frac=0.0,
               edge_frac=0.0, rand_angle_frac=0.1, tz=0.0, bf=synthetic.KITTI_BF, mp_fraction=0.9,
               obs_zero_fraction=0.1, outlier_fraction=0.03):
    """A SearchByProjection(Cur, Last) problem from numpy alone -> what frame_pair returns plus
    last_keys.  The last frame's keypoints are random, its map points are lifted at random depths;
    the current frame (rotated by synthetic.small_rotation, its centre moved tz along the optical
    axis: |tz| > bf / fx, 1.04 at 640 x 480, makes the stereo search a forward / backward one: see
    motion_of) holds their projections with 0.7 px noise and 6 % flipped descriptor bits, then
    unrelated keypoints, in shuffled order.
      pool > 0       descriptors are one of `pool` prototypes with 0-8 bits flipped: several
                     candidates at small distances in a window, exact ties included
      dup_frac       last keypoints that share position, octave, descriptor and map-point position
                     with another one: two queries contend for one current keypoint
      cluster_frac   current keypoints packed into grid cell (32, 24), the last keypoints they come
                     from moved so that they project within 6 px of it, half of them with the exact
                     descriptor and the angle of some last keypoint: windows of hundreds of candidates
      edge_frac      unrelated current keypoints outside the bounds and exactly on minX / maxX /
                     minY / maxY (each bound at least once when the share allows 4)
      rand_angle_frac  partners whose angle is random: the rotation histogram removes matches
      bounds         (minX, maxX, minY, maxY) of both frames; default the image"""
    K4 = synthetic.intrinsics(w, h)
    fx, fy, cx, cy = K4
    minX, maxX, minY, maxY = bounds if bounds is not None else (0.0, float(w), 0.0, float(h))
    cw, ch = (maxX - minX) / GRID_COLS, (maxY - minY) / GRID_ROWS
    scale = scale_factors()
    R = synthetic.small_rotation(rng, fx)
    Tcw = synthetic.pose_from_rotation(R, -R @ np.array([0.0, 0.0, tz]))
    protos = rng.integers(0, 256, (pool, 32), dtype=np.uint8) if pool > 0 else None
    octave_p = 0.7 ** np.arange(8)

    lk = _keys(n_last)
    lk["x"] = rng.uniform(2.0, w - 2.0, n_last)
    lk["y"] = rng.uniform(2.0, h - 2.0, n_last)
    lk["octave"] = rng.choice(8, n_last, p=octave_p / octave_p.sum())
    lk["angle"] = rng.uniform(0.0, 360.0, n_last)
    ld = _descriptors(rng, n_last, protos)
    n_dup = int(dup_frac * n_last) if n_last > 1 else 0
    order = rng.permutation(n_last)
    dup, orig = order[:n_dup], order[n_dup:]

    n_edge = int(edge_frac * n_cur)
    n_pair = min(len(orig), n_cur - n_edge - (n_cur // 12 if n_cur > 2 else 0))
    partner = orig[:n_pair]                       # last keypoint of current keypoint j < n_pair
    n_cl = int(round(cluster_frac * n_cur))
    in_cl = np.zeros(n_cur, bool)
    in_cl[rng.permutation(n_cur)[:n_cl]] = True
    cell = np.stack([minX + cw * (32 + rng.uniform(-0.4, 0.4, n_cur)), minY + ch * (24 + rng.uniform(-0.4, 0.4, n_cur))], 1)

    X = synthetic.lift_map_points(rng, lk, K4).astype(np.float64)
    clp = np.nonzero(in_cl[:n_pair])[0]           # clustered partners: the last keypoint moves under the cell
    if len(clp):
        tgt = cell[clp] + rng.uniform(-6.0, 6.0, (len(clp), 2))
        d = rng.uniform(5.0, 50.0, len(clp))
        ray = np.stack([(tgt[:, 0] - cx) / fx, (tgt[:, 1] - cy) / fy, np.ones(len(clp))], 1) * d[:, None]
        Xl = (ray - Tcw[:3, 3].astype(np.float64)) @ R       # R^T (Xc - t), world = the last camera
        X[partner[clp]] = Xl
        lk["x"][partner[clp]] = fx * Xl[:, 0] / Xl[:, 2] + cx
        lk["y"][partner[clp]] = fy * Xl[:, 1] / Xl[:, 2] + cy
    X = X.astype(np.float32)
    if n_dup:
        src = orig[rng.integers(0, len(orig), n_dup)]
        lk[dup] = lk[src]
        ld[dup] = ld[src]
        X[dup] = X[src]

    ck = _keys(n_cur)
    u, v, z = _project(Tcw, K4, X[partner])
    ck["x"][:n_pair] = u + rng.normal(0.0, 0.7, n_pair)
    ck["y"][:n_pair] = v + rng.normal(0.0, 0.7, n_pair)
    ck["octave"][:n_pair] = np.clip(lk["octave"][partner] + rng.choice([-1, 0, 0, 0, 1], n_pair), 0, 7)
    ang = lk["angle"][partner] + rng.normal(0.0, 2.0, n_pair)
    ang = np.where(rng.random(n_pair) < rand_angle_frac, rng.uniform(0.0, 360.0, n_pair), ang)
    ck["angle"][:n_pair] = np.mod(ang, 360.0)
    cd = np.empty((n_cur, 32), np.uint8)
    cd[:n_pair] = ld[partner] ^ np.packbits(rng.random((n_pair, 256)) < 0.06, axis=1)
    n_un = n_cur - n_pair
    ck["x"][n_pair:] = rng.uniform(2.0, w - 2.0, n_un)
    ck["y"][n_pair:] = rng.uniform(2.0, h - 2.0, n_un)
    ck["octave"][n_pair:] = rng.choice(8, n_un, p=octave_p / octave_p.sum())
    ck["angle"][n_pair:] = rng.uniform(0.0, 360.0, n_un)
    cd[n_pair:] = _descriptors(rng, n_un, protos)
    zc = np.concatenate([z, rng.uniform(5.0, 50.0, n_un)])

    ck["x"][in_cl] = cell[in_cl, 0]
    ck["y"][in_cl] = cell[in_cl, 1]
    copy = in_cl & (rng.random(n_cur) < 0.5)
    if n_last and copy.any():
        src = rng.integers(0, n_last, int(copy.sum()))
        cd[copy] = ld[src]
        ck["angle"][copy] = np.mod(lk["angle"][src] + rng.normal(0.0, 2.0, len(src)), 360.0)

    e = np.arange(n_cur - n_edge, n_cur)          # the last unrelated keypoints become edge keypoints
    for j, i in enumerate(e):
        side = j % 4
        if j < min(8, n_edge // 2):               # exactly on a bound, the other coordinate inside
            ck["x"][i] = (minX, maxX)[side] if side < 2 else rng.uniform(minX + cw, maxX - cw)
            ck["y"][i] = (minY, maxY)[side - 2] if side >= 2 else rng.uniform(minY + ch, maxY - ch)
        else:                                     # outside: at least 0.6 cells before min, any amount past max
            off = rng.uniform(0.6, 3.0)
            ck["x"][i] = (minX - off * cw, maxX + off * cw)[side] if side < 2 else rng.uniform(minX, maxX)
            ck["y"][i] = (minY - off * ch, maxY + off * ch)[side - 2] if side >= 2 else rng.uniform(minY, maxY)

    uR = None
    if stereo:
        uR = (ck["x"] - np.float32(bf) / zc + rng.normal(0.0, 0.3, n_cur)).astype(np.float32)
        uR = np.where(rng.random(n_cur) < 0.6, uR, -1).astype(np.float32)
    sh = rng.permutation(n_cur)
    ck, cd = ck[sh], cd[sh]
    if uR is not None:
        uR = uR[sh]

    bnd = dict(minX=minX, maxX=maxX, minY=minY, maxY=maxY)
    last = Frame(lk, ld, scale, np.eye(4, dtype=np.float32), fx, fy, cx, cy, bf if stereo else 0.0, w, h, **bnd)
    cur = Frame(ck, cd, scale, Tcw, fx, fy, cx, cy, bf if stereo else 0.0, w, h, uRight=uR, **bnd)
    mps = MapPoints(X, ld, np.where(rng.random(n_last) < obs_zero_fraction, 0, rng.integers(1, 6, n_last)))
    last_mp = np.where(rng.random(n_last) < mp_fraction, np.arange(n_last), -1).astype(np.int32)
    last_outlier = (rng.random(n_last) < outlier_fraction).astype(np.uint8)
    return cur, last, mps, last_mp, last_outlier, lk


def synth_local(rng, pair, nq, *, jitter=0.8, in_view_fraction=0.95, preset_fraction=0.15, fresh_tail=0,
                fresh_pool=0.25):
    """SearchByProjection(F, vpMapPoints, th) inputs for nq queries over a synth_pair problem ->
    (in_view, proj_x, proj_xr, proj_y, level, view_cos, mp_index, cur_mp).  The queries are drawn
    with repetition from the pair's map points; the projections carry `jitter` px of noise, the
    predicted level is the last keypoint's octave -1 / 0 / +1, a share is out of view and a share
    of cur_mp is preset.  fresh_tail > 0: the last fresh_tail queries are drawn from map points
    held out of the earlier ones (up to the share fresh_pool of the table), so that late queries
    still find their keypoint free."""
    cur, last, mps, last_mp, last_outlier, lk = pair
    n = mps.n
    K4 = (float(cur.fx), float(cur.fy), float(cur.cx), float(cur.cy))
    if n == 0:
        nq = 0
    held = rng.permutation(n)[:min(fresh_tail, int(n * fresh_pool))] if fresh_tail else np.zeros(0, np.int64)
    if len(held) == 0:
        fresh_tail = 0
    head = np.setdiff1d(np.arange(n), held)
    mp_index = np.concatenate([head[rng.integers(0, max(len(head), 1), nq - fresh_tail)] if nq - fresh_tail else head[:0],
                               held[rng.integers(0, max(len(held), 1), fresh_tail)] if fresh_tail else held[:0]])
    mp_index = mp_index.astype(np.int32)
    u, v, z = _project(cur.Tcw, K4, mps.pos[mp_index])
    px = (u + rng.normal(0.0, jitter, nq)).astype(np.float32)
    py = (v + rng.normal(0.0, jitter, nq)).astype(np.float32)
    pxr = (px - float(synthetic.KITTI_BF) / z + rng.normal(0.0, 0.3, nq)).astype(np.float32)
    level = np.clip(lk["octave"][mp_index] + rng.integers(-1, 2, nq), 0, len(cur.scale) - 1).astype(np.int32)
    view_cos = rng.uniform(0.99, 1.0, nq).astype(np.float32)
    in_view = ((rng.random(nq) < in_view_fraction) & (z > 0)).astype(np.uint8)
    cur_mp = np.full(cur.N, -1, np.int32)
    if n:
        cur_mp = np.where(rng.random(cur.N) < preset_fraction, rng.integers(0, n, cur.N), -1).astype(np.int32)
    return in_view, px, pxr, py, level, view_cos, mp_index, cur_mp


def empty_local_map():
    return dict(pos=np.zeros((0, 3), np.float32), desc=np.zeros((0, 32), np.uint8), obs=np.zeros(0, np.int32),
                max_dist=np.zeros(0, np.float32), min_dist=np.zeros(0, np.float32),
                normal=np.zeros((0, 3), np.float32), skip=np.zeros(0, np.uint8))


def synth_local_map(rng, pair, n_points, extra=300):
    """The local map dict SearchLocalPoints takes (local_map above) for a synth_pair problem:
    n_points - extra points lifted from the last frame's keypoints, drawn with repetition once
    there are more points than keypoints (several map points with one position and descriptor),
    plus `extra` points that fail isInFrustum.  Use pairs with tz = 0: the points are lifted at
    depths of their own."""
    cur, last, mps, last_mp, last_outlier, lk = pair
    n = n_points - extra
    if len(lk) == 0 or n <= 0:
        return empty_local_map()
    idx = rng.permutation(len(lk))[:n] if n <= len(lk) else rng.integers(0, len(lk), n)
    K4 = (float(cur.fx), float(cur.fy), float(cur.cx), float(cur.cy))
    return local_map(rng, lk[idx], mps.desc[idx], cur.scale, extra=extra, K4=K4)


# ------------------------------------------------------------------ the shape matrix
# One SearchByProjection(Cur, Last) problem of the matrix; MapPoints queries come from the same
# pair (local_of).  tags: "contended" (duplicates + prototypes at a size where 20 contended
# keypoints are possible at all: >= 1000 queries, 200 of them duplicates), "clustered", "edge".
PairCase = namedtuple("PairCase", "id seed n_last n_cur w h kw tags")

LADDER_N = (0, 1, 63, 1535, 1536, 1537, 2000, 4095, 4096)
STAGE_MAX_N = 1536        # kStageMaxN: above it the candidate search reads the frame from device memory
SLOT_QUERIES = 4096       # k_select_r<false>: queries beyond NT * Q go through qinfo
MAX_FRAME_KEYS = 4096     # kMaxFrameKeys
AMBIGUOUS = dict(pool=64, dup_frac=0.2)
GEOMETRIES = (("qvga", 320, 240, None), ("wvga", 752, 480, None), ("kitti-wide", 1241, 376, WIDE_BOUNDS))


def _pair_cases():
    cases, seed = [], 1000
    # the stereo rungs 1535 / 2000 / 4096 move forward and 1537 backward by 1.5 baselines
    # (bForward / bBackward, ORBmatcher.cc:1344-1345: one-sided level ranges); motion_of() restates the
    # test and tests/test_match_cases_cpu.py asserts it
    b = synthetic.KITTI_BF / synthetic.intrinsics(640, 480)[0]
    tz = {1535: 1.5 * b, 1537: -1.5 * b, 2000: 1.5 * b, 4096: 1.5 * b}
    for n in LADDER_N:
        for stereo in (False, True):
            seed += 1
            kw = dict(AMBIGUOUS, stereo=stereo, tz=tz.get(n, 0.0) if stereo else 0.0)
            n_last = n - n // 20
            tags = ("ladder",) + (("contended",) if n_last >= 1000 else ())
            cases.append(PairCase(f"ladder-{n}-{'stereo' if stereo else 'mono'}", seed, n_last, n, 640, 480, kw, tags))
    for n_last in (0, 1):   # no query / one query against an ordinary frame
        seed += 1
        cases.append(PairCase(f"last-{n_last}", seed, n_last, 300, 640, 480, dict(AMBIGUOUS), ("ladder",)))
    for name, w, h, bounds in GEOMETRIES:
        for n in (300, 2000):
            seed += 1
            kw = dict(AMBIGUOUS, bounds=bounds, edge_frac=0.1, stereo=n == 2000)
            cases.append(PairCase(f"geom-{name}-{n}", seed, n - n // 20, n, w, h, kw, ("geometry", "edge")))
    for n in (1536, 4096):
        for frac in (0.6, 1.0):
            seed += 1
            kw = dict(AMBIGUOUS, cluster_frac=frac)
            cases.append(PairCase(f"crowded-{n}-{frac}", seed, n - n // 20, n, 640, 480, kw, ("crowded", "clustered")))
    return cases


PAIR_CASES = _pair_cases()
PAIR_BY_ID = {c.id: c for c in PAIR_CASES}
LAST_TH = (7.0, 15.0)       # Tracking.cc:869-892
CROWDED_TH = (15.0, 100.0)
LOCAL_TH = (1.0, 5.0)       # Tracking.cc:1184-1191


@functools.lru_cache(maxsize=None)
def pair_of(case_id):
    """(cur, last, mps, last_mp, last_outlier, last_keys) of a PairCase or a mixed-batch / path frame, built once."""
    c = PAIR_BY_ID[case_id] if case_id in PAIR_BY_ID else EXTRA_PAIRS[case_id]
    return synth_pair(np.random.default_rng(c.seed), c.n_last, c.n_cur, c.w, c.h, **c.kw)


@functools.lru_cache(maxsize=None)
def local_of(case_id, nq=None, fresh_tail=0, fresh_pool=0.25):
    """synth_local queries over pair_of(case_id): nq defaults to the last frame's keypoint count."""
    pair = pair_of(case_id)
    c = PAIR_BY_ID[case_id] if case_id in PAIR_BY_ID else EXTRA_PAIRS[case_id]
    return synth_local(np.random.default_rng(c.seed + 50000 + (nq or 0)), pair, c.n_last if nq is None else nq,
                       fresh_tail=fresh_tail, fresh_pool=fresh_pool)


# frames used by the beyond-the-slots, mixed-batch and path cases
EXTRA_PAIRS = {
    "frame-1500": PairCase("frame-1500", 2001, 1425, 1500, 640, 480, dict(AMBIGUOUS, stereo=True), ()),
    "frame-2500": PairCase("frame-2500", 2002, 2375, 2500, 640, 480, dict(AMBIGUOUS), ()),
    "mix-300": PairCase("mix-300", 2003, 285, 300, 640, 480, dict(AMBIGUOUS), ()),
    "mix-1536a": PairCase("mix-1536a", 2004, 1460, 1536, 640, 480, dict(AMBIGUOUS), ()),
    "mix-1536b": PairCase("mix-1536b", 2005, 1460, 1536, 640, 480, dict(AMBIGUOUS, stereo=True), ()),
    "mix-1537": PairCase("mix-1537", 2006, 1461, 1537, 640, 480, dict(AMBIGUOUS), ()),
    "map-1500": PairCase("map-1500", 2007, 1425, 1500, 640, 480, dict(AMBIGUOUS, stereo=True), ()),
    "map-2500": PairCase("map-2500", 2008, 2375, 2500, 640, 480, dict(AMBIGUOUS), ()),
}
BEYOND_NQ = (4096, 4097, 4700, 9000)
BEYOND_FRAMES = ("frame-1500", "frame-2500")
MIXED_BATCHES = (("mix-300", "mix-1537"), ("mix-1536a", "mix-1536b"), ("mix-1536a", "mix-1537"))
BATCH_NP = (1, 7, 8, 9, 17)
LOCAL_MAP_POINTS = 5900     # synth_local_map: about 85 % of the 5,600 lifted points are in view
LOG_SCALE_FACTOR = np.float32(np.log(np.float32(1.2)))


@functools.lru_cache(maxsize=None)
def mixed_local_maps(ids):
    """The local maps of a mixed batch's SearchLocalPoints half: one per frame, 200 points more than
    the last frame has keypoints (so some are drawn twice), 100 of them failing isInFrustum."""
    rng = np.random.default_rng(77)
    return [synth_local_map(rng, pair_of(i), pair_of(i)[1].N + 200, extra=100) for i in ids]


def beyond_local(frame_id, nq):
    """MapPoints queries past the register slots: the queries from index 4096 on are fresh (synth_local)."""
    return local_of(frame_id, nq, max(nq - SLOT_QUERIES, 0))


@functools.lru_cache(maxsize=None)
def big_local_map(frame_id):
    """(frame, cur_mp, local map) with more than 4,600 in-view points over pair_of(frame_id)."""
    pair = pair_of(frame_id)
    rng = np.random.default_rng(EXTRA_PAIRS[frame_id].seed + 70000)
    M = synth_local_map(rng, pair, LOCAL_MAP_POINTS)
    cur = pair[0]
    cm = np.where(rng.random(cur.N) < 0.15, rng.integers(0, len(M["pos"]), cur.N), -1).astype(np.int32)
    M["skip"][cm[cm >= 0]] = 1            # points already in the frame (mnLastFrameSeen)
    return cur, cm, M


@functools.lru_cache(maxsize=None)
def batch_problems(np_):
    """np_ small problems for the batch tests: frame sizes cycle over 300, 0, 1, 200, the query
    counts differ, problem 2 (when there is one) has no query and problem 3 no in-view point.
    -> list of (pair, local map, cur_mp for SearchLocalPoints)."""
    out = []
    for p in range(np_):
        n_cur = (300, 0, 1, 200)[p % 4]
        n_last = 0 if p == 2 else (260, 40, 7, 180)[p % 4] + 3 * p
        rng = np.random.default_rng(3000 + 37 * np_ + p)
        pair = synth_pair(rng, n_last, n_cur, 640, 480, stereo=p % 3 == 1, **AMBIGUOUS)
        M = synth_local_map(rng, pair, 0 if p == 2 else n_last + 60 + 17 * p, extra=40)
        if p == 3:
            M["skip"][:] = 1
        cm = np.full(n_cur, -1, np.int32)
        if len(M["pos"]) and n_cur:
            cm = np.where(rng.random(n_cur) < 0.15, rng.integers(0, len(M["pos"]), n_cur), -1).astype(np.int32)
            M["skip"][cm[cm >= 0]] = 1
        out.append((pair, M, cm))
    return out


# ------------------------------------------------------------------ brute-force windows (numpy)
def _roundf(v):
    """C roundf: halves away from zero (np.rint rounds them to even)."""
    return np.copysign(np.floor(np.abs(v) + np.float32(0.5)), v)


def _in_grid(F):
    """Keypoints AssignFeaturesToGrid keeps (PosInGrid, Frame.cc:382-392), in float as the reference."""
    px = _roundf((F.keysUn["x"] - F.minX) * F.gridWInv)
    py = _roundf((F.keysUn["y"] - F.minY) * F.gridHInv)
    return (px >= 0) & (px < GRID_COLS) & (py >= 0) & (py < GRID_ROWS)


def _window_mask(F, x, y, r, lo, hi):
    """[query, keypoint]: the keypoint passes the reference's radius and level-range tests."""
    k = F.keysUn
    o = k["octave"][None, :]
    return ((np.abs(k["x"][None, :] - x[:, None]) < r[:, None]) & (np.abs(k["y"][None, :] - y[:, None]) < r[:, None]) &
            (o >= lo[:, None]) & (o <= hi[:, None]) & _in_grid(F)[None, :])


def motion_of(pair, bMono):
    """(bForward, bBackward) of SearchByProjection(Cur, Last), ORBmatcher.cc:1338-1345: tlc = Rlw twc + tlw,
    with twc and tlc rounded to float as cv::Mat products are."""
    cur, last = pair[0], pair[1]
    Tc, Tl = cur.Tcw.astype(np.float64), last.Tcw.astype(np.float64)
    twc = (-(Tc[:3, :3].T @ Tc[:3, 3])).astype(np.float32).astype(np.float64)
    tlc_z = np.float32(Tl[2, :3] @ twc + Tl[2, 3])
    return bool(tlc_z > cur.b) and not bMono, bool(-tlc_z > cur.b) and not bMono


def last_windows(pair, th, bMono):
    """Brute-force windows of SearchByProjection(Cur, Last): -> (query indices, mask[query, keypoint])."""
    cur, last, mps, last_mp, last_outlier, lk = pair
    q = np.nonzero((last_mp >= 0) & (last_outlier == 0))[0]
    K4 = (float(cur.fx), float(cur.fy), float(cur.cx), float(cur.cy))
    u, v, z = _project(cur.Tcw, K4, mps.pos[last_mp[q]])
    ok = (z > 0) & (u >= cur.minX) & (u <= cur.maxX) & (v >= cur.minY) & (v <= cur.maxY)
    q, u, v = q[ok], u[ok], v[ok]
    oc = lk["octave"][q].astype(np.int64)
    fwd, bwd = motion_of(pair, bMono)
    lo, hi = (oc, oc * 0 + 99) if fwd else (oc * 0, oc) if bwd else (oc - 1, oc + 1)
    return q, _window_mask(cur, u, v, th * cur.scale[oc].astype(np.float64), lo, hi)


def local_windows(pair, loc, th):
    """Brute-force windows of SearchByProjection(F, vpMapPoints, th): -> (query indices, mask)."""
    cur = pair[0]
    in_view, px, pxr, py, level, view_cos, mp_index, cur_mp = loc
    q = np.nonzero(in_view)[0]
    r = np.where(view_cos[q] > 0.998, 2.5, 4.0) * th * cur.scale[level[q]]
    return q, _window_mask(cur, px[q].astype(np.float64), py[q].astype(np.float64), r, level[q] - 1, level[q])


def hamming(a, b):
    if not hasattr(np, "bitwise_count"):   # numpy < 2
        return np.unpackbits(np.ascontiguousarray(a) ^ np.ascontiguousarray(b), axis=1).sum(axis=1).astype(np.int64)
    x = np.ascontiguousarray(a).view(np.uint64) ^ np.ascontiguousarray(b).view(np.uint64)
    return np.bitwise_count(x).sum(axis=1).astype(np.int64)


def contended_keypoints(qdesc, kdesc, mask):
    """Keypoints that are the nearest-descriptor candidate of two or more queries."""
    qi, ki = np.nonzero(mask)
    if len(qi) == 0:
        return 0
    d = hamming(qdesc[qi], kdesc[ki])
    order = np.lexsort((d, qi))
    first = np.concatenate([[True], qi[order][1:] != qi[order][:-1]])
    return int((np.bincount(ki[order][first], minlength=len(kdesc)) >= 2).sum())
