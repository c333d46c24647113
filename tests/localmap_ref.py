"""Scalar restatement of LocalMapping::CreateNewMapPoints' per-pair geometry and of the two
MapPoint updates, in exactly the operation order of c_orb_slam_amd/csrc/localmap.hip, plus a
float64 reference with plain formulas.

A float32 value is held as the Python float it equals.  F() rounds a double to float32; for one
+, -, *, / or sqrt on float32 operands the double result rounded by F() is the correctly
rounded float32 result (53 >= 2 * 24 + 2), so `F(a * b)` is the device's float multiply and a
bare Python expression is the device's double arithmetic.
"""
import math
import struct

import numpy as np

_pack, _unpack = struct.Struct("f").pack, struct.Struct("f").unpack
FLT_EPSILON = 2.0 ** -23


def F(x):
    return _unpack(_pack(x))[0]


# ---- detmath.hpp ---------------------------------------------------------------------------
def sincos_d(x):
    S1, S2, S3 = -1.66666666666666324348e-01, 8.33333333332248946124e-03, -1.98412698298579493134e-04
    S4, S5, S6 = 2.75573137070700676789e-06, -2.50507602534068634195e-08, 1.58969099521155010221e-10
    C1, C2, C3 = 4.16666666666666019037e-02, -1.38888888888741095749e-03, 2.48015872894767294178e-05
    C4, C5, C6 = -2.75573143513906633035e-07, 2.08757232129817482790e-09, -1.13596475577881948265e-11
    pio2_1, pio2_1t = 1.57079632673412561417e+00, 6.07710050650619224932e-11
    invpio2 = 6.36619772367581382433e-01
    fn = float(round(x * invpio2))          # rint: half to even
    n = int(fn)
    y = (x - fn * pio2_1) - fn * pio2_1t
    z = y * y
    r = S2 + z * (S3 + z * (S4 + z * (S5 + z * S6)))
    s = y + (z * y) * (S1 + z * r)
    rc = z * (C1 + z * (C2 + z * (C3 + z * (C4 + z * (C5 + z * C6)))))
    c = 1.0 - (0.5 * z - z * rc)
    return ((s, c), (c, -s), (-s, -c), (-c, s))[n & 3]


def _atan01(x):
    x = x / (1.0 + math.sqrt(1.0 + x * x))
    x = x / (1.0 + math.sqrt(1.0 + x * x))
    x2 = x * x
    term = total = x
    for k in range(1, 15):
        term = term * x2
        total += (-term if k & 1 else term) / (2 * k + 1)
    return 4.0 * total


def atan2_d(y, x):
    ay, ax = abs(y), abs(x)
    if ax == 0 and ay == 0:
        a = 0.0
    elif ay <= ax:
        a = _atan01(ay / ax)
    else:
        a = 1.57079632679489655800e+00 - _atan01(ax / ay)
    if x < 0:
        a = 3.14159265358979311600e+00 - a
    return -a if y < 0 else a


# ---- OpenCV 3.2 JacobiSVDImpl_<float>, 4 x 4, vt.row(3) only -----------------------------------
def svd4_vt3(At):
    """At: 4 x 4 list of float32 values (the transposed A); -> vt.row(3)."""
    At = [list(r) for r in At]
    eps = 2 * FLT_EPSILON
    W = [0.0] * 4
    Vt = [[1.0 if k == i else 0.0 for k in range(4)] for i in range(4)]
    for i in range(4):
        sd = 0.0
        for k in range(4):
            sd += At[i][k] * At[i][k]
        W[i] = sd
    for _ in range(30):
        changed = False
        for i in range(3):
            for j in range(i + 1, 4):
                a, b, p = W[i], W[j], 0.0
                for k in range(4):
                    p += At[i][k] * At[j][k]
                if abs(p) <= eps * math.sqrt(a * b):
                    continue
                p *= 2
                beta = a - b
                gamma = math.sqrt(p * p + beta * beta)
                if beta < 0:
                    delta = (gamma - beta) * 0.5
                    s = math.sqrt(delta / gamma)
                    c = p / (gamma * s * 2)
                else:
                    c = math.sqrt((gamma + beta) / (gamma * 2))
                    s = p / (gamma * c * 2)
                a = b = 0.0
                for k in range(4):
                    t0 = F(c * At[i][k] + s * At[j][k])
                    t1 = F(-s * At[i][k] + c * At[j][k])
                    At[i][k], At[j][k] = t0, t1
                    a += t0 * t0
                    b += t1 * t1
                W[i], W[j] = a, b
                changed = True
                for k in range(4):
                    t0 = F(c * Vt[i][k] + s * Vt[j][k])
                    t1 = F(-s * Vt[i][k] + c * Vt[j][k])
                    Vt[i][k], Vt[j][k] = t0, t1
        if not changed:
            break
    for i in range(4):
        sd = 0.0
        for k in range(4):
            sd += At[i][k] * At[i][k]
        W[i] = math.sqrt(sd)
    for i in range(3):
        j = i
        for k in range(i + 1, 4):
            if W[j] < W[k]:
                j = k
        if i != j:
            W[i], W[j] = W[j], W[i]
            Vt[i], Vt[j] = Vt[j], Vt[i]
    return Vt[3]


# ---- keyframes -------------------------------------------------------------------------------
class KF:
    """The keyframe fields CreateNewMapPoints reads, as float32-valued Python floats."""

    def __init__(self, frame, depth, sigma2):
        self.T = [float(v) for v in np.asarray(frame.Tcw, np.float32).ravel()[:12]]
        self.fx, self.fy, self.cx, self.cy = (float(v) for v in (frame.fx, frame.fy, frame.cx, frame.cy))
        self.bf, self.b = float(frame.bf), float(frame.b)
        self.invfx, self.invfy = F(1.0 / self.fx), F(1.0 / self.fy)
        self.sf = [float(v) for v in frame.scale]
        self.sigma2 = [float(v) for v in np.asarray(sigma2, np.float32)]
        self.x = [float(v) for v in frame.keysUn["x"]]
        self.y = [float(v) for v in frame.keysUn["y"]]
        self.oct = [int(v) for v in frame.keysUn["octave"]]
        self.ur = None if frame.uRight is None else [float(v) for v in frame.uRight]
        self.depth = None if depth is None else [float(v) for v in np.asarray(depth, np.float32)]
        T = self.T
        # Rwc = Rcw^T, Ow = -Rwc * tcw (gemm with alpha -1)
        self.Twc = [0.0] * 12
        for r in range(3):
            for c in range(3):
                self.Twc[r * 4 + c] = T[c * 4 + r]
            s = (T[r] * T[3] + T[4 + r] * T[7]) + T[8 + r] * T[11]
            self.Twc[r * 4 + 3] = F(s * -1.0)


def _cam_row(T, r, X):
    d = (T[r * 4] * X[0] + T[r * 4 + 1] * X[1]) + T[r * 4 + 2] * X[2]
    return F(d + T[r * 4 + 3])


def _norm3(v):
    return math.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])


def _cos_parallax_stereo(b, depth):
    a = atan2_d(F(b / 2), depth)
    return F(sincos_d(2.0 * a)[1])


def _unproject(Twc, u, v, z, K):
    x = F(F(F(u - K.cx) * z) * K.invfx)
    y = F(F(F(v - K.cy) * z) * K.invfy)
    return [F(((Twc[r * 4] * x + Twc[r * 4 + 1] * y) + Twc[r * 4 + 2] * z) + Twc[r * 4 + 3]) for r in range(3)]


def _reproj_fails(K, X, z, kx, ky, kur, stereo, sigma2):
    x, y = _cam_row(K.T, 0, X), _cam_row(K.T, 1, X)
    invz = F(1.0 / z)
    u = F(F(F(K.fx * x) * invz) + K.cx)
    v = F(F(F(K.fy * y) * invz) + K.cy)
    ex, ey = F(u - kx), F(v - ky)
    e2 = F(F(ex * ex) + F(ey * ey))
    if not stereo:
        return e2 > 5.991 * sigma2
    ur = F(u - F(K.bf * invz))
    er = F(ur - kur)
    return F(e2 + F(er * er)) > 7.8 * sigma2


def restate_pair(K1, K2, i1, i2, scaleFactor):
    """-> (status, x3D, normal, max_dist, min_dist); the last four None for status <= 0."""
    T1, T2 = K1.T, K2.T
    x1, y1, x2, y2 = K1.x[i1], K1.y[i1], K2.x[i2], K2.y[i2]
    ur1 = K1.ur[i1] if K1.ur is not None else -1.0
    ur2 = K2.ur[i2] if K2.ur is not None else -1.0
    xn1 = [F(F(x1 - K1.cx) * K1.invfx), F(F(y1 - K1.cy) * K1.invfy), 1.0]
    xn2 = [F(F(x2 - K2.cx) * K2.invfx), F(F(y2 - K2.cy) * K2.invfy), 1.0]
    ray1 = [F((K1.Twc[r * 4] * xn1[0] + K1.Twc[r * 4 + 1] * xn1[1]) + K1.Twc[r * 4 + 2] * xn1[2]) for r in range(3)]
    ray2 = [F((K2.Twc[r * 4] * xn2[0] + K2.Twc[r * 4 + 1] * xn2[1]) + K2.Twc[r * 4 + 2] * xn2[2]) for r in range(3)]
    dot = (ray1[0] * ray2[0] + ray1[1] * ray2[1]) + ray1[2] * ray2[2]
    cpr = F(dot / (_norm3(ray1) * _norm3(ray2)))
    st1, st2 = ur1 >= 0, ur2 >= 0
    cps1 = cps2 = F(cpr + 1)
    if st1:
        cps1 = _cos_parallax_stereo(K1.b, K1.depth[i1])
    elif st2:
        cps2 = _cos_parallax_stereo(K2.b, K2.depth[i2])
    cps = cps2 if cps2 < cps1 else cps1
    none = (None, None, None, None)
    if cpr < cps and cpr > 0 and (st1 or st2 or cpr < 0.9998):
        At = [[F(F(xn1[0] * T1[8 + k]) - T1[k]), F(F(xn1[1] * T1[8 + k]) - T1[4 + k]),
               F(F(xn2[0] * T2[8 + k]) - T2[k]), F(F(xn2[1] * T2[8 + k]) - T2[4 + k])] for k in range(4)]
        h = svd4_vt3(At)
        if h[3] == 0:
            return (-1,) + none
        inv = F(1.0 / h[3])
        X = [F(h[r] * inv) for r in range(3)]
        st = 1
    elif st1 and cps1 < cps2:
        X = _unproject(K1.Twc, x1, y1, K1.depth[i1], K1)
        st = 2
    elif st2 and cps2 < cps1:
        X = _unproject(K2.Twc, x2, y2, K2.depth[i2], K2)
        st = 3
    else:
        return (0,) + none
    z1 = _cam_row(T1, 2, X)
    if z1 <= 0:
        return (-2,) + none
    z2 = _cam_row(T2, 2, X)
    if z2 <= 0:
        return (-4,) + none
    o1, o2 = K1.oct[i1], K2.oct[i2]
    if _reproj_fails(K1, X, z1, x1, y1, ur1, st1, K1.sigma2[o1]):
        return (-3,) + none
    if _reproj_fails(K2, X, z2, x2, y2, ur2, st2, K2.sigma2[o2]):
        return (-5,) + none
    n1 = [F(X[r] - K1.Twc[r * 4 + 3]) for r in range(3)]
    n2 = [F(X[r] - K2.Twc[r * 4 + 3]) for r in range(3)]
    nd1, nd2 = _norm3(n1), _norm3(n2)
    dist1, dist2 = F(nd1), F(nd2)
    if dist1 == 0 or dist2 == 0:
        return (-6,) + none
    ratioDist = F(dist2 / dist1)
    ratioOctave = F(K1.sf[o1] / K2.sf[o2])
    ratioFactor = F(1.5 * scaleFactor)
    if F(ratioDist * ratioFactor) < ratioOctave or ratioDist > F(ratioOctave * ratioFactor):
        return (-7,) + none
    i1n, i2n = F(1.0 / nd1), F(1.0 / nd2)
    normal = [F(F(F(0.0 + F(n1[r] * i1n)) + F(n2[r] * i2n)) * 0.5) for r in range(3)]
    mx = F(dist1 * K1.sf[o1])
    return st, X, normal, mx, F(mx / K1.sf[-1])


def restate_batch(KF1, depth1, sigma2_1, scaleFactor, neighbours):
    """The restatement in ORBmatcher.CreateNewMapPoints' input and output layout."""
    K1 = KF(KF1, depth1, sigma2_1)
    sfac = float(np.float32(scaleFactor))
    outs = []
    for KF2, depth2, sigma2_2, pairs in neighbours:
        K2 = KF(KF2, depth2, sigma2_2)
        pairs = np.asarray(pairs, np.int32).reshape(-1, 2)
        n = len(pairs)
        x3D, status = np.zeros((n, 3), np.float32), np.zeros(n, np.int8)
        normal, mx, mn = np.zeros((n, 3), np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32)
        for i, (i1, i2) in enumerate(pairs):
            st, X, nr, a, b = restate_pair(K1, K2, int(i1), int(i2), sfac)
            status[i] = st
            if st > 0:
                x3D[i], normal[i], mx[i], mn[i] = X, nr, a, b
        outs.append((x3D, status, normal, mx, mn))
    return outs


# ---- float64 reference --------------------------------------------------------------------------
def ref64_pair(T1, T2, cam1, cam2, kp1, kp2, sf1, sf2, sig1, sig2, scaleFactor):
    """Plain float64 formulas.  T: 4x4; cam: (fx, fy, cx, cy, bf, b); kp: (x, y, uRight, depth,
    octave).  -> (status, x3D or None, borderline)."""
    T1, T2 = np.asarray(T1, np.float64), np.asarray(T2, np.float64)
    border = False

    def near(a, b, tol):                     # absolute
        return abs(a - b) < tol

    def nearrel(a, b):                       # relative 1e-3 of the threshold b
        return abs(a - b) <= 1e-3 * abs(b)

    R1, t1, R2, t2 = T1[:3, :3], T1[:3, 3], T2[:3, :3], T2[:3, 3]
    O1, O2 = -R1.T @ t1, -R2.T @ t2
    (fx1, fy1, cx1, cy1, bf1, b1), (fx2, fy2, cx2, cy2, bf2, b2) = cam1, cam2
    x1, y1, ur1, d1, o1 = kp1
    x2, y2, ur2, d2, o2 = kp2
    xn1 = np.array([(x1 - cx1) / fx1, (y1 - cy1) / fy1, 1.0])
    xn2 = np.array([(x2 - cx2) / fx2, (y2 - cy2) / fy2, 1.0])
    ray1, ray2 = R1.T @ xn1, R2.T @ xn2
    cpr = float(ray1 @ ray2 / (np.linalg.norm(ray1) * np.linalg.norm(ray2)))
    st1, st2 = ur1 >= 0, ur2 >= 0
    cps1 = cps2 = cpr + 1
    if st1:
        cps1 = math.cos(2 * math.atan2(b1 / 2, d1))
    elif st2:
        cps2 = math.cos(2 * math.atan2(b2 / 2, d2))
    cps = min(cps1, cps2)
    border |= near(cpr, cps, 2e-6) or near(cpr, 0.0, 2e-6)
    if not (st1 or st2):
        border |= near(cpr, 0.9998, 2e-6)
    if cpr < cps and cpr > 0 and (st1 or st2 or cpr < 0.9998):
        A = np.stack([xn1[0] * T1[2] - T1[0], xn1[1] * T1[2] - T1[1], xn2[0] * T2[2] - T2[0], xn2[1] * T2[2] - T2[1]])
        h = np.linalg.svd(A)[2][3]
        if h[3] == 0:
            return -1, None, border
        X = h[:3] / h[3]
        st = 1
    elif st1 and cps1 < cps2:
        border |= near(cps1, cps2, 2e-6)
        X = R1.T @ (xn1 * d1) + O1
        st = 2
    elif st2 and cps2 < cps1:
        border |= near(cps1, cps2, 2e-6)
        X = R2.T @ (xn2 * d2) + O2
        st = 3
    else:
        if st1 or st2:
            border |= near(cps1, cps2, 2e-6)
        return 0, None, border
    c1, c2 = R1 @ X + t1, R2 @ X + t2
    nx = float(np.linalg.norm(X))
    border |= abs(c1[2]) < 1e-4 * nx
    if c1[2] <= 0:
        return -2, None, border
    border |= abs(c2[2]) < 1e-4 * nx
    if c2[2] <= 0:
        return -4, None, border

    def chi(c, fx, fy, cx, cy, bf, x, y, ur, stereo, s2):
        u, v = fx * c[0] / c[2] + cx, fy * c[1] / c[2] + cy
        e2 = (u - x) ** 2 + (v - y) ** 2
        if not stereo:
            return e2, 5.991 * s2
        return e2 + (u - bf / c[2] - ur) ** 2, 7.8 * s2

    e, th = chi(c1, fx1, fy1, cx1, cy1, bf1, x1, y1, ur1, st1, sig1[o1])
    border |= nearrel(e, th)
    if e > th:
        return -3, None, border
    e, th = chi(c2, fx2, fy2, cx2, cy2, bf2, x2, y2, ur2, st2, sig2[o2])
    border |= nearrel(e, th)
    if e > th:
        return -5, None, border
    dist1, dist2 = float(np.linalg.norm(X - O1)), float(np.linalg.norm(X - O2))
    if dist1 == 0 or dist2 == 0:
        return -6, None, border
    ratioDist, ratioOctave, rf = dist2 / dist1, sf1[o1] / sf2[o2], 1.5 * scaleFactor
    border |= nearrel(ratioDist * rf, ratioOctave) or nearrel(ratioDist, ratioOctave * rf)
    if ratioDist * rf < ratioOctave or ratioDist > ratioOctave * rf:
        return -7, None, border
    return st, X, border


# ---- MapPoint updates ---------------------------------------------------------------------------
_POP = np.array([bin(i).count("1") for i in range(256)], np.uint8)


def hamming_matrix(desc):
    d = np.asarray(desc, np.uint8).reshape(-1, 32)
    return _POP[d[:, None, :] ^ d[None, :, :]].sum(axis=2, dtype=np.int32)


def _select16(row, first, step, need):
    for c in range(16):
        if int((row <= first + step * c).sum()) >= need:
            return c
    return 16


def restate_best(desc):
    """ComputeDistinctiveDescriptors as the device computes it: per row the smallest v with
    #{D[i][j] <= v} >= m + 1, by a counting select in two passes (thresholds 15, 31, .., 255,
    then the 16 values of that bucket; 256 when no bucket reaches the count), and the least
    (median, index)."""
    k = len(desc)
    if k == 0:
        return -1
    D = hamming_matrix(desc)
    need = (k - 1) // 2 + 1
    best = None
    for i in range(k):
        median = 256
        bucket = _select16(D[i], 15, 16, need)
        if bucket < 16:
            median = 16 * bucket + _select16(D[i], 16 * bucket, 1, need)
        if best is None or (median, i) < best:
            best = (median, i)
    return best[1]


def brute_best(desc):
    """The reference's loop: sort each row, take element 0.5 * (k - 1), strict '<' against INT_MAX."""
    k = len(desc)
    if k == 0:
        return -1
    D = hamming_matrix(desc)
    best_median, best_idx = 2 ** 31 - 1, 0
    for i in range(k):
        median = int(np.sort(D[i])[int(0.5 * (k - 1))])
        if median < best_median:
            best_median, best_idx = median, i
    return best_idx


def restate_normal_depth(pos, obs_Ow, ref_Ow, ref_scale, ref_scale_top):
    """UpdateNormalAndDepth of one point: -> (normal[3], max_dist, min_dist) as float32 values."""
    X = [float(v) for v in np.asarray(pos, np.float32)]
    acc = [0.0, 0.0, 0.0]
    Ow = np.asarray(obs_Ow, np.float32).reshape(-1, 3)
    for O in Ow:
        v = [F(X[r] - float(O[r])) for r in range(3)]
        inv = F(1.0 / _norm3(v))
        acc = [F(acc[r] + F(v[r] * inv)) for r in range(3)]
    invn = F(1.0 / float(len(Ow)))
    normal = [F(acc[r] * invn) for r in range(3)]
    R = [float(v) for v in np.asarray(ref_Ow, np.float32)]
    dist = F(_norm3([F(X[r] - R[r]) for r in range(3)]))
    mx = F(dist * float(np.float32(ref_scale)))
    return normal, mx, F(mx / float(np.float32(ref_scale_top)))


def ref64_normal_depth(pos, obs_Ow, ref_Ow, ref_scale, ref_scale_top):
    X = np.asarray(pos, np.float64)
    v = X - np.asarray(obs_Ow, np.float64).reshape(-1, 3)
    normal = (v / np.linalg.norm(v, axis=1)[:, None]).mean(axis=0)
    mx = float(np.linalg.norm(X - np.asarray(ref_Ow, np.float64))) * float(ref_scale)
    return normal, mx, mx / float(ref_scale_top)
