"""Scalar restatement of ORB_SLAM2::Initializer (src/Initializer.cc) in exactly the operation
order of c_orb_slam_amd/csrc/initializer.hip and capi_initializer.cpp, plus a float64 reference
with plain formulas (np.linalg.svd, the same RANSAC sets, the same acceptance rules).

Conventions as in localmap_ref.py: a float32 value is held as the Python float it equals, F()
rounds a double to float32, a bare Python expression is the device's double arithmetic.  The
per-match checks run on float32 NumPy arrays: every elementwise +, -, *, / there is one
correctly rounded float32 operation, the same as the scalar code.
"""
import math

import numpy as np

import localmap_ref
from localmap_ref import FLT_EPSILON, atan2_d, svd4_vt3

FLT_MIN = 2.0 ** -126
f32 = np.float32


def F(x):
    """Round to float32; beyond FLT_MAX the result is an infinity, as on the device."""
    try:
        return localmap_ref.F(x)
    except OverflowError:
        return math.copysign(math.inf, x)


# ---- glibc rand() (TYPE_3) and DUtils::Random::RandomInt ---------------------------------------
class GlibcRand:
    """srand(seed); rand().  count = draws so far."""

    def __init__(self, seed):
        seed = (seed & 0xFFFFFFFF) or 1
        r = [seed if seed < 2 ** 31 else seed - 2 ** 32]
        for _ in range(30):
            hi = r[-1] // 127773 if r[-1] >= 0 else -((-r[-1]) // 127773)
            lo = r[-1] - hi * 127773
            w = 16807 * lo - 2836 * hi
            if w < 0:
                w += 2147483647
            r.append(w)
        r += r[0:3]
        self.r = [v & 0xFFFFFFFF for v in r]
        for _ in range(310):
            self._next()
        self.count = 0

    def _next(self):
        v = (self.r[-31] + self.r[-3]) & 0xFFFFFFFF
        self.r.append(v)
        del self.r[0]
        return v

    def rand(self):
        self.count += 1
        return self._next() >> 1


def random_int(rng, mn, mx):
    return int((rng.rand() / (2147483647 + 1.0)) * (mx - mn + 1)) + mn


def draw_sets(rng, N, iterations):
    """Initializer::Initialize's mvSets: 8 swap-remove draws per iteration from 0..N-1."""
    sets = []
    for _ in range(iterations):
        avail = list(range(N))
        s = []
        for _ in range(8):
            r = random_int(rng, 0, len(avail) - 1)
            s.append(avail[r])
            avail[r] = avail[-1]
            avail.pop()
        sets.append(s)
    return sets


# ---- small CV_32F matrix operations (OpenCV semantics) ------------------------------------------
def _div(a, b):
    try:
        return a / b
    except ZeroDivisionError:
        if a != a or a == 0:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)


def mm(A, B, alpha=1.0):
    """gemm: A (r x k) * B (k x c), each element accumulated in double in k order, times alpha,
    rounded once."""
    k = len(B)
    out = []
    for row in A:
        o = []
        for c in range(len(B[0])):
            acc = 0.0
            for q in range(k):
                acc = acc + row[q] * B[q][c]
            o.append(F(acc * alpha))
        out.append(o)
    return out


def tr(A):
    return [list(r) for r in zip(*A)]


def det3(m):
    return (m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0])
            + m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]))


def inv3(S):
    d = det3(S)
    if d == 0:
        return [[0.0] * 3 for _ in range(3)]
    d = _div(1.0, d)
    t = [(S[1][1] * S[2][2] - S[1][2] * S[2][1]) * d, (S[0][2] * S[2][1] - S[0][1] * S[2][2]) * d,
         (S[0][1] * S[1][2] - S[0][2] * S[1][1]) * d, (S[1][2] * S[2][0] - S[1][0] * S[2][2]) * d,
         (S[0][0] * S[2][2] - S[0][2] * S[2][0]) * d, (S[0][2] * S[1][0] - S[0][0] * S[1][2]) * d,
         (S[1][0] * S[2][1] - S[1][1] * S[2][0]) * d, (S[0][1] * S[2][0] - S[0][0] * S[2][1]) * d,
         (S[0][0] * S[1][1] - S[0][1] * S[1][0]) * d]
    return [[F(t[3 * r + c]) for c in range(3)] for r in range(3)]


def norm_d(v):
    s = 0.0
    for x in v:
        s = s + x * x
    return math.sqrt(s)


def _sqrtf(x):
    return F(math.sqrt(x)) if x >= 0 else math.nan


def acos_d(x):
    """acos through detmath's atan2_d: atan2(sqrt((1 - x)(1 + x)), x)."""
    q = (1.0 - x) * (1.0 + x)
    return atan2_d(math.sqrt(q) if q >= 0 else math.nan, x)   # |x| > 1: NaN, as acos


# ---- OpenCV 3.2 JacobiSVDImpl_<float> ----------------------------------------------------------
class _CvRng:
    def __init__(self):
        self.s = 0x12345678

    def next(self):
        self.s = ((self.s & 0xFFFFFFFF) * 4164903690 + (self.s >> 32)) & 0xFFFFFFFFFFFFFFFF
        return self.s & 0xFFFFFFFF


def jacobi_svd(At, m, n, n1, want_vt=True, normalise=True):
    """At: n1 rows of length m (rows n.. zero), float32 values; the rows 0..n-1 are orthogonalised.
    -> (W as doubles, At, Vt).  oracle/linalg.c:27-140 with float storage: W, the dot products
    and the rotation scalars in double, rotated and scaled entries rounded to float."""
    At = [list(r) for r in At]
    eps = 2 * FLT_EPSILON
    W = [0.0] * n
    Vt = [[1.0 if k == i else 0.0 for k in range(n)] for i in range(n)] if want_vt else None
    for i in range(n):
        sd = 0.0
        for k in range(m):
            sd += At[i][k] * At[i][k]
        W[i] = sd
    for _ in range(max(m, 30)):
        changed = False
        for i in range(n - 1):
            for j in range(i + 1, n):
                Ai, Aj = At[i], At[j]
                a, b, p = W[i], W[j], 0.0
                for k in range(m):
                    p += Ai[k] * Aj[k]
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
                for k in range(m):
                    t0 = F(c * Ai[k] + s * Aj[k])
                    t1 = F(-s * Ai[k] + c * Aj[k])
                    Ai[k], Aj[k] = t0, t1
                    a += t0 * t0
                    b += t1 * t1
                W[i], W[j] = a, b
                changed = True
                if Vt is not None:
                    Vi, Vj = Vt[i], Vt[j]
                    for k in range(n):
                        t0 = F(c * Vi[k] + s * Vj[k])
                        t1 = F(-s * Vi[k] + c * Vj[k])
                        Vi[k], Vj[k] = t0, t1
        if not changed:
            break
    for i in range(n):
        sd = 0.0
        for k in range(m):
            sd += At[i][k] * At[i][k]
        W[i] = math.sqrt(sd)
    for i in range(n - 1):
        j = i
        for k in range(i + 1, n):
            if W[j] < W[k]:
                j = k
        if i != j:
            W[i], W[j] = W[j], W[i]
            At[i], At[j] = At[j], At[i]
            if Vt is not None:
                Vt[i], Vt[j] = Vt[j], Vt[i]
    if not normalise:
        return W, At, Vt
    rng = _CvRng()
    for i in range(n1):
        sd = W[i] if i < n else 0.0
        ii = 0
        while ii < 100 and sd <= FLT_MIN:
            val0 = F(1.0 / m)
            for k in range(m):
                At[i][k] = val0 if (rng.next() & 256) != 0 else -val0
            for _ in range(2):
                for j in range(i):
                    sd = 0.0
                    for k in range(m):
                        sd += At[i][k] * At[j][k]
                    asum = 0.0
                    for k in range(m):
                        t = F(At[i][k] - sd * At[j][k])
                        At[i][k] = t
                        asum += abs(t)
                    asum = 1 / asum if asum > eps * 100 else 0.0
                    for k in range(m):
                        At[i][k] = F(At[i][k] * asum)
            sd = 0.0
            for k in range(m):
                sd += At[i][k] * At[i][k]
            sd = math.sqrt(sd)
            ii += 1
        s = 1 / sd if sd > FLT_MIN else 0.0
        for k in range(m):
            At[i][k] = F(At[i][k] * s)
    return W, At, Vt


def svd3(A):
    """cv::SVD::compute(A, w, u, vt, FULL_UV) of a 3 x 3 CV_32F matrix -> (w, u, vt)."""
    W, At, Vt = jacobi_svd(tr(A), 3, 3, 3)
    return [F(x) for x in W], tr(At), Vt


# ---- Normalize ------------------------------------------------------------------------------------
def normalize(keys):
    """Initializer::Normalize over all keys of a frame -> (points n x 2 float32, T 3 x 3)."""
    keys = np.asarray(keys, f32).reshape(-1, 2)
    n = len(keys)
    xs, ys = [float(v) for v in keys[:, 0]], [float(v) for v in keys[:, 1]]
    mx = my = 0.0
    for i in range(n):
        mx = F(mx + xs[i])
        my = F(my + ys[i])
    mx, my = F(_div(mx, float(n))), F(_div(my, float(n)))
    dx = dy = 0.0
    px, py = [0.0] * n, [0.0] * n
    for i in range(n):
        px[i], py[i] = F(xs[i] - mx), F(ys[i] - my)
        dx = F(dx + abs(px[i]))
        dy = F(dy + abs(py[i]))
    dx, dy = F(_div(dx, float(n))), F(_div(dy, float(n)))
    sX, sY = F(_div(1.0, dx)), F(_div(1.0, dy))
    with np.errstate(all="ignore"):
        pts = np.stack([np.array(px, f32) * f32(sX), np.array(py, f32) * f32(sY)], axis=1)
        T = [[sX, 0.0, float(f32(-mx) * f32(sX))], [0.0, sY, float(f32(-my) * f32(sY))], [0.0, 0.0, 1.0]]
    return pts, T


# ---- hypotheses -----------------------------------------------------------------------------------
def compute_h21(p1, p2):
    """p1, p2: 8 normalised points each -> Hn 3 x 3 (vt.row(8) of the 16 x 9 system)."""
    A = []
    for (u1, v1), (u2, v2) in zip(p1, p2):
        A.append([0.0, 0.0, 0.0, -u1, -v1, -1.0, F(v2 * u1), F(v2 * v1), v2])
        A.append([u1, v1, 1.0, 0.0, 0.0, 0.0, -F(u2 * u1), -F(u2 * v1), -u2])
    _, _, Vt = jacobi_svd(tr(A), 16, 9, 9, normalise=False)
    h = Vt[8]
    return [h[0:3], h[3:6], h[6:9]]


def compute_f21(p1, p2):
    A = []
    for (u1, v1), (u2, v2) in zip(p1, p2):
        A.append([F(u2 * u1), F(u2 * v1), u2, F(v2 * u1), F(v2 * v1), v2, u1, v1, 1.0])
    A.append([0.0] * 9)
    # m < n: OpenCV works on A itself (8 rows of length 9), n1 = 9; row 8 is the completion
    _, At, _ = jacobi_svd(A, 9, 8, 9, want_vt=False)
    f = At[8]
    w, u, vt = svd3([f[0:3], f[3:6], f[6:9]])
    w[2] = 0.0
    D = [[w[0], 0.0, 0.0], [0.0, w[1], 0.0], [0.0, 0.0, w[2]]]
    return mm(mm(u, D), vt)


def _seq_sum(t1, t2):
    s = 0.0
    for a, b in zip(t1.tolist(), t2.tolist()):
        s = F(s + a)
        s = F(s + b)
    return s


def check_homography(H21, H12, px, sigma):
    """px: N x 4 float32 (u1, v1, u2, v2) -> (score, inlier mask)."""
    h = [[f32(v) for v in r] for r in H21]
    hi = [[f32(v) for v in r] for r in H12]
    u1, v1, u2, v2 = px[:, 0], px[:, 1], px[:, 2], px[:, 3]
    th = f32(5.991)
    inv_s2 = f32(_div(1.0, F(sigma * sigma)))
    with np.errstate(all="ignore"):
        w = f32(1) / (hi[2][0] * u2 + hi[2][1] * v2 + hi[2][2])
        a = (hi[0][0] * u2 + hi[0][1] * v2 + hi[0][2]) * w
        b = (hi[1][0] * u2 + hi[1][1] * v2 + hi[1][2]) * w
        chi1 = ((u1 - a) * (u1 - a) + (v1 - b) * (v1 - b)) * inv_s2
        w = f32(1) / (h[2][0] * u1 + h[2][1] * v1 + h[2][2])
        a = (h[0][0] * u1 + h[0][1] * v1 + h[0][2]) * w
        b = (h[1][0] * u1 + h[1][1] * v1 + h[1][2]) * w
        chi2 = ((u2 - a) * (u2 - a) + (v2 - b) * (v2 - b)) * inv_s2
        out1, out2 = chi1 > th, chi2 > th
        t1 = np.where(out1, f32(0), th - chi1).astype(f32)
        t2 = np.where(out2, f32(0), th - chi2).astype(f32)
    return _seq_sum(t1, t2), ~(out1 | out2)


def check_fundamental(F21, px, sigma):
    f = [[f32(v) for v in r] for r in F21]
    u1, v1, u2, v2 = px[:, 0], px[:, 1], px[:, 2], px[:, 3]
    th, th_score = f32(3.841), f32(5.991)
    inv_s2 = f32(_div(1.0, F(sigma * sigma)))
    with np.errstate(all="ignore"):
        a2 = f[0][0] * u1 + f[0][1] * v1 + f[0][2]
        b2 = f[1][0] * u1 + f[1][1] * v1 + f[1][2]
        c2 = f[2][0] * u1 + f[2][1] * v1 + f[2][2]
        num2 = a2 * u2 + b2 * v2 + c2
        chi1 = (num2 * num2 / (a2 * a2 + b2 * b2)) * inv_s2
        a1 = f[0][0] * u2 + f[1][0] * v2 + f[2][0]
        b1 = f[0][1] * u2 + f[1][1] * v2 + f[2][1]
        c1 = f[0][2] * u2 + f[1][2] * v2 + f[2][2]
        num1 = a1 * u1 + b1 * v1 + c1
        chi2 = (num1 * num1 / (a1 * a1 + b1 * b1)) * inv_s2
        out1, out2 = chi1 > th, chi2 > th
        t1 = np.where(out1, f32(0), th_score - chi1).astype(f32)
        t2 = np.where(out2, f32(0), th_score - chi2).astype(f32)
    return _seq_sum(t1, t2), ~(out1 | out2)


# ---- CheckRT --------------------------------------------------------------------------------------
def _is_finite(x):
    return x == x and abs(x) != math.inf


def check_rt(R, t, K, px, first, inliers, n1, th2):
    """-> (nGood, parallax, vP3D n1 x 3 float32, vbGood n1 bool)."""
    fx, fy, cx, cy = K[0][0], K[1][1], K[0][2], K[1][2]
    P1 = [K[r] + [0.0] for r in range(3)]
    P2 = mm(K, [R[r] + [t[r]] for r in range(3)])
    O2 = [v[0] for v in mm(tr(R), [[t[0]], [t[1]], [t[2]]], -1.0)]
    vP3D, vbGood = np.zeros((n1, 3), f32), np.zeros(n1, bool)
    cosines = []
    for i in range(len(px)):
        if not inliers[i]:
            continue
        u1, v1, u2, v2 = (float(v) for v in px[i])
        At = [[F(F(u1 * P1[2][k]) - P1[0][k]), F(F(v1 * P1[2][k]) - P1[1][k]),
               F(F(u2 * P2[2][k]) - P2[0][k]), F(F(v2 * P2[2][k]) - P2[1][k])] for k in range(4)]
        h = svd4_vt3(At)
        inv = F(_div(1.0, h[3]))
        X = [F(h[r] * inv) for r in range(3)]
        if not (_is_finite(X[0]) and _is_finite(X[1]) and _is_finite(X[2])):
            continue
        dist1 = F(norm_d(X))
        n2 = [F(X[r] - O2[r]) for r in range(3)]
        dist2 = F(norm_d(n2))
        dot = (X[0] * n2[0] + X[1] * n2[1]) + X[2] * n2[2]
        cosp = F(_div(dot, F(dist1 * dist2)))
        if cosp != cosp:
            continue                          # the reference's sort is undefined on a NaN
        if X[2] <= 0 and cosp < 0.99998:
            continue
        X2 = [F(((R[r][0] * X[0] + R[r][1] * X[1]) + R[r][2] * X[2]) + t[r]) for r in range(3)]
        if X2[2] <= 0 and cosp < 0.99998:
            continue
        invz = F(_div(1.0, X[2]))
        ex = F(F(F(F(fx * X[0]) * invz) + cx) - u1)
        ey = F(F(F(F(fy * X[1]) * invz) + cy) - v1)
        if F(F(ex * ex) + F(ey * ey)) > th2:
            continue
        invz = F(_div(1.0, X2[2]))
        ex = F(F(F(F(fx * X2[0]) * invz) + cx) - u2)
        ey = F(F(F(F(fy * X2[1]) * invz) + cy) - v2)
        if F(F(ex * ex) + F(ey * ey)) > th2:
            continue
        cosines.append(cosp)
        vP3D[first[i]] = X
        vbGood[first[i]] = cosp < 0.99998
    nGood = len(cosines)
    parallax = 0.0
    if nGood > 0:
        c = sorted(cosines)[min(50, nGood - 1)]
        parallax = F(acos_d(c) * 180 / 3.1415926535897932384626433832795)
    return nGood, parallax, vP3D, vbGood


# ---- motion hypotheses ----------------------------------------------------------------------------
def _unit(t):
    inv = F(_div(1.0, norm_d(t)))
    return [F(v * inv) for v in t]


def decompose_e(E):
    w, u, vt = svd3(E)
    t = _unit([u[0][2], u[1][2], u[2][2]])
    Wm = [[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]
    R1 = mm(mm(u, Wm), vt)
    if det3(R1) < 0:
        R1 = [[-v for v in r] for r in R1]
    R2 = mm(mm(u, tr(Wm)), vt)
    if det3(R2) < 0:
        R2 = [[-v for v in r] for r in R2]
    return R1, R2, t


def motions_f(F21, K):
    E = mm(mm(tr(K), F21), K)
    R1, R2, t = decompose_e(E)
    tn = [-v for v in t]
    return [(R1, t), (R2, t), (R1, tn), (R2, tn)]


def motions_h(H21, K):
    """The eight Faugeras hypotheses, or [] when the singular values are too close."""
    A = mm(mm(inv3(K), H21), K)
    w, U, Vt = svd3(A)
    s = F(det3(U) * det3(Vt))
    d1, d2, d3 = w
    if F(_div(d1, d2)) < 1.00001 or F(_div(d2, d3)) < 1.00001:
        return []
    q1, q2, q3 = F(d1 * d1), F(d2 * d2), F(d3 * d3)
    den = F(q1 - q3)
    aux1 = _sqrtf(F(_div(F(q1 - q2), den)))
    aux3 = _sqrtf(F(_div(F(q2 - q3), den)))
    x1 = [aux1, aux1, -aux1, -aux1]
    x3 = [aux3, -aux3, aux3, -aux3]
    prod = F(F(q1 - q2) * F(q2 - q3))
    root = _sqrtf(prod)
    out = []
    for case in range(2):
        if case == 0:
            den2 = F(F(d1 + d3) * d2)
            sn = F(_div(root, den2))
            cs = F(_div(F(q2 + F(d1 * d3)), den2))
            scale = F(d1 - d3)
        else:
            den2 = F(F(d1 - d3) * d2)
            sn = F(_div(root, den2))
            cs = F(_div(F(F(d1 * d3) - q2), den2))
            scale = F(d1 + d3)
        sns = [sn, -sn, -sn, sn]
        for i in range(4):
            if case == 0:
                Rp = [[cs, 0.0, -sns[i]], [0.0, 1.0, 0.0], [sns[i], 0.0, cs]]
                tp = [F(x1[i] * scale), 0.0, F(-x3[i] * scale)]
            else:
                Rp = [[cs, 0.0, sns[i]], [0.0, -1.0, 0.0], [sns[i], 0.0, -cs]]
                tp = [F(x1[i] * scale), 0.0, F(x3[i] * scale)]
            R = mm(mm(U, Rp, s), Vt)
            t = [v[0] for v in mm(U, [[tp[0]], [tp[1]], [tp[2]]])]
            out.append((R, _unit(t)))
    return out


# ---- Initialize -----------------------------------------------------------------------------------
class Initializer:
    def __init__(self, K, keys1, sigma=1.0, iterations=200):
        self.K = [[float(v) for v in r] for r in np.asarray(K, f32).reshape(3, 3)]
        self.keys1 = np.asarray(keys1, f32).reshape(-1, 2)
        self.sigma = float(f32(sigma))
        self.iterations = int(iterations)
        self.pn1, self.T1 = normalize(self.keys1)

    def Initialize(self, keys2, matches12, rng):
        """-> dict(ok, R21, t21, vP3D, vbTriangulated, info); rng: GlibcRand, advanced by 8 * iterations."""
        keys2 = np.asarray(keys2, f32).reshape(-1, 2)
        m12 = np.asarray(matches12, np.int32)
        n1 = len(self.keys1)
        first = np.nonzero(m12 >= 0)[0]
        second = m12[first]
        N = len(first)
        px = np.concatenate([self.keys1[first], keys2[second]], axis=1).astype(f32)
        pn2, T2 = normalize(keys2)
        T2inv, T2t = inv3(T2), tr(T2)
        pa = [(float(a), float(b)) for a, b in self.pn1[first]]
        pb = [(float(a), float(b)) for a, b in pn2[second]]
        sets = draw_sets(rng, N, self.iterations)
        info = dict(SH=0.0, SF=0.0, best_it_H=-1, best_it_F=-1, H21=np.zeros(9, f32), F21=np.zeros(9, f32),
                    inliersH=np.zeros(N, bool), inliersF=np.zeros(N, bool), n_hyp=0, nGood=[0] * 8,
                    parallax=[0.0] * 8, chosen=-1)
        H21 = F21 = None
        for it, s in enumerate(sets):
            p1, p2 = [pa[j] for j in s], [pb[j] for j in s]
            Hi = mm(mm(T2inv, compute_h21(p1, p2)), self.T1)
            sc, inl = check_homography(Hi, inv3(Hi), px, self.sigma)
            if sc > info["SH"]:
                info.update(SH=sc, best_it_H=it, inliersH=inl)
                H21 = Hi
            Fi = mm(mm(T2t, compute_f21(p1, p2)), self.T1)
            sc, inl = check_fundamental(Fi, px, self.sigma)
            if sc > info["SF"]:
                info.update(SF=sc, best_it_F=it, inliersF=inl)
                F21 = Fi
        if H21 is not None:
            info["H21"] = np.array(H21, f32).ravel()
        if F21 is not None:
            info["F21"] = np.array(F21, f32).ravel()
        RH = F(_div(info["SH"], F(info["SH"] + info["SF"])))
        use_H = RH > float(f32(0.40))
        info["use_H"] = int(use_H)
        model, inl = (H21, info["inliersH"]) if use_H else (F21, info["inliersF"])
        res = dict(ok=False, R21=None, t21=None, vP3D=None, vbTriangulated=None, info=info)
        # why: the first acceptance rule that failed ("" on success); not a device output
        info["why"] = ""
        if model is None:
            info["why"] = "no model"
            return res
        motions = motions_h(model, self.K) if use_H else motions_f(model, self.K)
        info["n_hyp"] = len(motions)
        if not motions:
            info["why"] = "gate"
            return res
        th2 = F(4.0 * F(self.sigma * self.sigma))
        Nin = int(np.count_nonzero(inl))
        checks = [check_rt(R, t, self.K, px, first, inl, n1, th2) for R, t in motions]
        for k, c in enumerate(checks):
            info["nGood"][k], info["parallax"][k] = c[0], c[1]
        good = [c[0] for c in checks]
        chosen = -1
        if use_H:
            best = second = 0
            bi, bpar = -1, -1.0
            for k, c in enumerate(checks):
                if c[0] > best:
                    second, best, bi, bpar = best, c[0], k, c[1]
                elif c[0] > second:
                    second = c[0]
            if not second < 0.75 * best:
                info["why"] = "second best"
            elif not bpar >= 1.0:
                info["why"] = "parallax"
            elif not (best > 50 and best > 0.9 * Nin):
                info["why"] = "few"
            else:
                chosen = bi
        else:
            mx = max(good)
            n_min = max(int(0.9 * Nin), 50)
            nsimilar = sum(1 for g in good if g > 0.7 * mx)
            info["nsimilar"] = nsimilar
            if mx < n_min:
                info["why"] = "few"
            elif nsimilar > 1:
                info["why"] = "nsimilar"
            else:
                k = good.index(mx)
                if checks[k][1] > 1.0:
                    chosen = k
                else:
                    info["why"] = "parallax"
        info["chosen"] = chosen
        if chosen >= 0:
            R, t = motions[chosen]
            res.update(ok=True, R21=np.array(R, f32), t21=np.array(t, f32), vP3D=checks[chosen][2],
                       vbTriangulated=checks[chosen][3])
        return res


# ---- float64 reference ----------------------------------------------------------------------------
def _normalize64(keys):
    k = np.asarray(keys, np.float64).reshape(-1, 2)
    mean = k.mean(axis=0)
    s = 1.0 / np.abs(k - mean).mean(axis=0)
    T = np.array([[s[0], 0, -mean[0] * s[0]], [0, s[1], -mean[1] * s[1]], [0, 0, 1.0]])
    return (k - mean) * s, T


def _chi_h64(H21, px, sigma):
    H12 = np.linalg.inv(H21)
    x1 = np.concatenate([px[:, 0:2], np.ones((len(px), 1))], axis=1)
    x2 = np.concatenate([px[:, 2:4], np.ones((len(px), 1))], axis=1)
    a, b = x2 @ H12.T, x1 @ H21.T
    c1 = ((x1[:, :2] - a[:, :2] / a[:, 2:3]) ** 2).sum(axis=1) / sigma ** 2
    c2 = ((x2[:, :2] - b[:, :2] / b[:, 2:3]) ** 2).sum(axis=1) / sigma ** 2
    return np.stack([c1, c2], axis=1)


def _chi_f64(F21, px, sigma):
    x1 = np.concatenate([px[:, 0:2], np.ones((len(px), 1))], axis=1)
    x2 = np.concatenate([px[:, 2:4], np.ones((len(px), 1))], axis=1)
    l2, l1 = x1 @ F21.T, x2 @ F21
    c1 = (l2 * x2).sum(axis=1) ** 2 / (l2[:, 0] ** 2 + l2[:, 1] ** 2) / sigma ** 2
    c2 = (l1 * x1).sum(axis=1) ** 2 / (l1[:, 0] ** 2 + l1[:, 1] ** 2) / sigma ** 2
    return np.stack([c1, c2], axis=1)


def _score64(chi, th, th_score):
    return float(np.where(chi > th, 0.0, th_score - chi).sum()), ~(chi > th).any(axis=1)


def _check_rt64(R, t, K, px, first, inl, n1, th2):
    P1 = np.concatenate([K, np.zeros((3, 1))], axis=1)
    P2 = K @ np.concatenate([R, t.reshape(3, 1)], axis=1)
    O2 = -R.T @ t
    X3, good, cosines = np.zeros((n1, 3)), np.zeros(n1, bool), []
    for i in np.nonzero(inl)[0]:
        u1, v1, u2, v2 = px[i]
        A = np.stack([u1 * P1[2] - P1[0], v1 * P1[2] - P1[1], u2 * P2[2] - P2[0], v2 * P2[2] - P2[1]])
        v = np.linalg.svd(A)[2][3]
        with np.errstate(all="ignore"):
            X = v[:3] / v[3]
        if not np.all(np.isfinite(X)):
            continue
        n2 = X - O2
        cosp = float(X @ n2 / (np.linalg.norm(X) * np.linalg.norm(n2)))
        if X[2] <= 0 and cosp < 0.99998:
            continue
        X2 = R @ X + t
        if X2[2] <= 0 and cosp < 0.99998:
            continue
        p1 = K @ X / X[2]
        if (p1[0] - u1) ** 2 + (p1[1] - v1) ** 2 > th2:
            continue
        p2 = K @ X2 / X2[2]
        if (p2[0] - u2) ** 2 + (p2[1] - v2) ** 2 > th2:
            continue
        cosines.append(cosp)
        X3[first[i]] = X
        good[first[i]] = cosp < 0.99998
    par = 0.0
    if cosines:
        par = math.degrees(math.acos(min(1.0, sorted(cosines)[min(50, len(cosines) - 1)])))
    return len(cosines), par, X3, good


def ref64_initialize(K, keys1, keys2, matches12, sets, sigma=1.0):
    """Initializer::Initialize in float64 with plain formulas on the given RANSAC sets.
    -> dict(ok, use_H, best_it_H, best_it_F, inliersH, inliersF, chiH, chiF (N x 2 chi-squares of
    the winners), R21, t21, vP3D, vbTriangulated, chosen)."""
    K = np.asarray(K, np.float64).reshape(3, 3)
    k1, k2 = np.asarray(keys1, np.float64).reshape(-1, 2), np.asarray(keys2, np.float64).reshape(-1, 2)
    m12 = np.asarray(matches12)
    first = np.nonzero(m12 >= 0)[0]
    second = m12[first]
    px = np.concatenate([k1[first], k2[second]], axis=1)
    N, n1 = len(first), len(k1)
    pn1, T1 = _normalize64(k1)
    pn2, T2 = _normalize64(k2)
    pa, pb = pn1[first], pn2[second]
    SH = SF = 0.0
    out = dict(ok=False, best_it_H=-1, best_it_F=-1, inliersH=np.zeros(N, bool), inliersF=np.zeros(N, bool),
               chiH=np.full((N, 2), np.inf), chiF=np.full((N, 2), np.inf), chosen=-1)
    H21 = F21 = None
    for it, s in enumerate(sets):
        A = []
        for (u1, v1), (u2, v2) in zip(pa[s], pb[s]):
            A.append([0, 0, 0, -u1, -v1, -1, v2 * u1, v2 * v1, v2])
            A.append([u1, v1, 1, 0, 0, 0, -u2 * u1, -u2 * v1, -u2])
        Hi = np.linalg.inv(T2) @ np.linalg.svd(np.array(A))[2][8].reshape(3, 3) @ T1
        with np.errstate(all="ignore"):
            chi = _chi_h64(Hi, px, sigma) if abs(np.linalg.det(Hi)) > 0 else np.full((N, 2), np.inf)
        sc, inl = _score64(chi, 5.991, 5.991)
        if sc > SH:
            SH, H21 = sc, Hi
            out.update(best_it_H=it, inliersH=inl, chiH=chi)
        A = [[u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, 1] for (u1, v1), (u2, v2) in zip(pa[s], pb[s])]
        u, w, vt = np.linalg.svd(np.linalg.svd(np.array(A))[2][8].reshape(3, 3))
        w[2] = 0
        Fi = T2.T @ (u @ np.diag(w) @ vt) @ T1
        with np.errstate(all="ignore"):
            chi = _chi_f64(Fi, px, sigma)
        sc, inl = _score64(chi, 3.841, 5.991)
        if sc > SF:
            SF, F21 = sc, Fi
            out.update(best_it_F=it, inliersF=inl, chiF=chi)
    RH = SH / (SH + SF) if SH + SF > 0 else math.nan
    use_H = RH > 0.40
    out.update(use_H=int(use_H), SH=SH, SF=SF)
    model, inl = (H21, out["inliersH"]) if use_H else (F21, out["inliersF"])
    if model is None:
        return out
    motions = []
    if use_H:
        U, w, Vt = np.linalg.svd(np.linalg.inv(K) @ model @ K)
        s = np.linalg.det(U) * np.linalg.det(Vt)
        d1, d2, d3 = w
        if d1 / d2 < 1.00001 or d2 / d3 < 1.00001:
            return out
        aux1 = math.sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3))
        aux3 = math.sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3))
        x1, x3 = [aux1, aux1, -aux1, -aux1], [aux3, -aux3, aux3, -aux3]
        root = math.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3))
        for case in range(2):
            if case == 0:
                sn, cs = root / ((d1 + d3) * d2), (d2 * d2 + d1 * d3) / ((d1 + d3) * d2)
            else:
                sn, cs = root / ((d1 - d3) * d2), (d1 * d3 - d2 * d2) / ((d1 - d3) * d2)
            for i, si in enumerate([sn, -sn, -sn, sn]):
                if case == 0:
                    Rp = np.array([[cs, 0, -si], [0, 1, 0], [si, 0, cs]])
                    tp = (d1 - d3) * np.array([x1[i], 0, -x3[i]])
                else:
                    Rp = np.array([[cs, 0, si], [0, -1, 0], [si, 0, -cs]])
                    tp = (d1 + d3) * np.array([x1[i], 0, x3[i]])
                t = U @ tp
                motions.append((s * U @ Rp @ Vt, t / np.linalg.norm(t)))
    else:
        u, w, vt = np.linalg.svd(K.T @ model @ K)
        t = u[:, 2] / np.linalg.norm(u[:, 2])
        Wm = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1.0]])
        R1, R2 = u @ Wm @ vt, u @ Wm.T @ vt
        R1 = -R1 if np.linalg.det(R1) < 0 else R1
        R2 = -R2 if np.linalg.det(R2) < 0 else R2
        motions = [(R1, t), (R2, t), (R1, -t), (R2, -t)]
    checks = [_check_rt64(R, t, K, px, first, inl, n1, 4.0 * sigma * sigma) for R, t in motions]
    good, Nin = [c[0] for c in checks], int(np.count_nonzero(inl))
    out.update(nGood=good, parallax=[c[1] for c in checks])
    chosen = -1
    if use_H:
        best = second_best = 0
        bi, bpar = -1, -1.0
        for k, c in enumerate(checks):
            if c[0] > best:
                second_best, best, bi, bpar = best, c[0], k, c[1]
            elif c[0] > second_best:
                second_best = c[0]
        if second_best < 0.75 * best and bpar >= 1.0 and best > 50 and best > 0.9 * Nin:
            chosen = bi
    else:
        mx = max(good)
        if not (mx < max(int(0.9 * Nin), 50) or sum(1 for g in good if g > 0.7 * mx) > 1):
            k = good.index(mx)
            if checks[k][1] > 1.0:
                chosen = k
    out["chosen"] = chosen
    if chosen >= 0:
        out.update(ok=True, R21=motions[chosen][0], t21=motions[chosen][1], vP3D=checks[chosen][2],
                   vbTriangulated=checks[chosen][3])
    return out
