"""Scalar restatement of LoopClosing's two map-moving steps in the reference's own order -- the first half
of LoopClosing::CorrectLoop and the tail of LoopClosing::RunGlobalBundleAdjustment (src/LoopClosing.cc) --
over the literal relation of tests/map_ref.py (RefMap), plus a float64 model with plain formulas.

Conventions (see localmap_ref.py): a float32 value is held as the Python float it equals, F() rounds a
double to float32, a bare Python expression is double arithmetic.  A cv::Mat product is one gemm: float
operands, the sum over k ascending in double, one rounding.  A Sim3 is the list [qx, qy, qz, qw, tx, ty,
tz, s] of doubles (g2o::Sim3; the layout of essgraph_problem); its product, inverse and map are the
operation sequences of c_orb_slam_amd/csrc/sim3_math.hpp.

The restatement walks the keyframes one after another as the reference does: a keyframe's points are
corrected, then its pose is set, so a later keyframe's points see the new pose of an earlier one.  The
library states the same thing as a rule ('listed and processed before the corrector'); the two are
independent formulations of one behaviour."""
import math

import numpy as np

from localmap_ref import F, _norm3, restate_normal_depth

BRANCHES = [0, 0, 0, 0]      # quat_from_R: trace > 0, then largest diagonal entry 0 / 1 / 2


# ---- cv::Mat helpers ---------------------------------------------------------------------------
def gemm(A, B, n=4):
    """A (4 x 4) * B (4 x n), row-major lists of float32 values."""
    return [F(((A[r * 4] * B[c] + A[r * 4 + 1] * B[n + c]) + A[r * 4 + 2] * B[2 * n + c]) + A[r * 4 + 3] * B[3 * n + c])
            for r in range(4) for c in range(n)]


def centre(T):
    """KeyFrame::SetPose: Ow = -Rwc * tcw, a gemm with alpha -1."""
    return [F(((T[r] * T[3] + T[4 + r] * T[7]) + T[8 + r] * T[11]) * -1.0) for r in range(3)]


def twc(T):
    Ow = centre(T)
    W = [0.0] * 16
    for r in range(3):
        for c in range(3):
            W[r * 4 + c] = T[c * 4 + r]
        W[r * 4 + 3] = Ow[r]
    W[15] = 1.0
    return W


def rot_apply(T, X):
    """R * X + t as one gemm (rows 0..2 of the 4 x 4 T)."""
    return [F(((T[r * 4] * X[0] + T[r * 4 + 1] * X[1]) + T[r * 4 + 2] * X[2]) + T[r * 4 + 3]) for r in range(3)]


# ---- g2o::Sim3 ---------------------------------------------------------------------------------
def quat_from_R(m):
    """Eigen's Quaterniond(Matrix3d), not normalised; m row-major 9 doubles -> [x, y, z, w]."""
    q = [0.0] * 4
    t = (m[0] + m[4]) + m[8]
    if t > 0:
        BRANCHES[0] += 1
        t = math.sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0] = (m[7] - m[5]) * t
        q[1] = (m[2] - m[6]) * t
        q[2] = (m[3] - m[1]) * t
    else:
        i = 0
        if m[4] > m[0]:
            i = 1
        if m[8] > m[i * 4]:
            i = 2
        BRANCHES[1 + i] += 1
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = math.sqrt(((m[i * 4] - m[j * 4]) - m[k * 4]) + 1.0)
        q[i] = 0.5 * t
        t = 0.5 / t
        q[3] = (m[k * 3 + j] - m[j * 3 + k]) * t
        q[j] = (m[j * 3 + i] + m[i * 3 + j]) * t
        q[k] = (m[k * 3 + i] + m[i * 3 + k]) * t
    return q


def quat_to_R(q):
    x, y, z, w = q
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return [1.0 - (tyy + tzz), txy - twz, txz + twy,
            txy + twz, 1.0 - (txx + tzz), tyz - twx,
            txz - twy, tyz + twx, 1.0 - (txx + tyy)]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def quat_rotate(q, v):
    uv = _cross(q, v)
    uv = [u + u for u in uv]
    c = _cross(q, uv)
    return [(v[i] + q[3] * uv[i]) + c[i] for i in range(3)]


def sim3_of_pose(T):
    """g2o::Sim3(toMatrix3d(R), toVector3d(t), 1.0) of a float 4 x 4."""
    return quat_from_R([T[r * 4 + c] for r in range(3) for c in range(3)]) + [T[3], T[7], T[11], 1.0]


def sim3_mul(a, b):
    w = ((a[3] * b[3] - a[0] * b[0]) - a[1] * b[1]) - a[2] * b[2]
    x = ((a[3] * b[0] + a[0] * b[3]) + a[1] * b[2]) - a[2] * b[1]
    y = ((a[3] * b[1] + a[1] * b[3]) + a[2] * b[0]) - a[0] * b[2]
    z = ((a[3] * b[2] + a[2] * b[3]) + a[0] * b[1]) - a[1] * b[0]
    rt = quat_rotate(a[:4], b[4:7])
    return [x, y, z, w] + [a[7] * rt[i] + a[4 + i] for i in range(3)] + [a[7] * b[7]]


def sim3_inverse(T):
    q = [-T[0], -T[1], -T[2], T[3]]
    ms = -1.0 / T[7]
    return q + quat_rotate(q, [ms * T[4], ms * T[5], ms * T[6]]) + [1.0 / T[7]]


def sim3_map(T, X):
    r = quat_rotate(T[:4], X)
    return [T[7] * r[i] + T[4 + i] for i in range(3)]


def pose_of_sim3(S):
    """[R | t * (1 / s); 0 0 0 1] with one cast per entry (Converter::toCvSE3 of the Eigen values)."""
    R = quat_to_R(S[:4])
    T = [0.0] * 16
    for r in range(3):
        for c in range(3):
            T[r * 4 + c] = F(R[r * 3 + c])
        T[r * 4 + 3] = F(S[4 + r] * (1.0 / S[7]))
    T[15] = 1.0
    return T


# ---- LoopClosing::CorrectLoop -------------------------------------------------------------------
def _rows16(a):
    return [[float(v) for v in row] for row in np.asarray(a, np.float32).reshape(-1, 16)]


def restate_correct_loop(ref, octaves, kf, cur_kf, Scw, scale_factors, Tcw, pos, normal, max_dist, min_dist,
                         ref_kf, corrected_ref, bad=None):
    """ref: RefMap; octaves: keyframe id -> per-slot octave.  The tables are not modified; -> dict with the
    new Tcw, pos, normal, max_dist, min_dist, corrected_ref (numpy, the tables' dtypes), CorrectedSim3 /
    NonCorrectedSim3 (nkf x 8 float64, in the order of kf), n_corrected, n_ref_missing."""
    T = _rows16(Tcw)
    pos = np.array(pos, np.float32).reshape(-1, 3)
    normal = np.array(normal, np.float32).reshape(-1, 3)
    max_dist, min_dist = np.array(max_dist, np.float32), np.array(min_dist, np.float32)
    corrected_ref = np.array(corrected_ref, np.int32)
    sf = [float(v) for v in np.asarray(scale_factors, np.float32)]
    Scw = [float(v) for v in Scw]
    Twc = twc(T[cur_kf])
    Corrected, NonCorrected = {cur_kf: Scw}, {}
    for i in kf:                                         # from the old poses
        i = int(i)
        if i != cur_kf:
            Sic = sim3_of_pose(gemm(T[i], Twc))
            Corrected[i] = sim3_mul(Sic, Scw)
        NonCorrected[i] = sim3_of_pose(T[i])
    done = set()                                         # mnCorrectedByKF == mpCurrentKF->mnId
    n_missing = 0
    for i in sorted(Corrected):                          # the KeyFrameAndPose map: id for address order
        Swi = sim3_inverse(Corrected[i])
        Siw = NonCorrected[i]
        for pMP in ref.kfs[i].mvpMapPoints:
            if pMP is None or pMP.isBad():
                continue
            p = pMP.mnId
            if p >= len(pos) or (bad is not None and bad[p]) or p in done:
                continue
            X = [F(v) for v in sim3_map(Swi, sim3_map(Siw, [float(v) for v in pos[p]]))]
            pos[p] = X
            done.add(p)
            corrected_ref[p] = i
            # MapPoint::UpdateNormalAndDepth with the poses as they are now
            obs = sorted(pMP.mObservations.items(), key=lambda kv: kv[0].mnId)
            if not obs:
                continue
            r = int(ref_kf[p])
            slot = {k.mnId: idx for k, idx in obs}.get(r)
            if slot is None or octaves[r][slot] >= len(sf):
                n_missing += 1
                continue
            nr, mx, mn = restate_normal_depth(X, [centre(T[k.mnId]) for k, _ in obs], centre(T[r]),
                                              sf[octaves[r][slot]], sf[-1])
            normal[p], max_dist[p], min_dist[p] = nr, mx, mn
        T[i] = pose_of_sim3(Corrected[i])                # pKFi->SetPose(correctedTiw)
    return dict(Tcw=np.array(T, np.float32), pos=pos, normal=normal, max_dist=max_dist, min_dist=min_dist,
                corrected_ref=corrected_ref, CorrectedSim3=np.array([Corrected[int(i)] for i in kf], np.float64),
                NonCorrectedSim3=np.array([NonCorrected[int(i)] for i in kf], np.float64), n_corrected=len(done),
                n_ref_missing=n_missing)


# ---- LoopClosing::RunGlobalBundleAdjustment, after Optimizer::GlobalBundleAdjustemnt ---------------
def restate_apply_gba(ref, origins, TcwGBA, kf_in_gba, Tcw, pos, posGBA, mp_in_gba, ref_kf, bad=None):
    """-> dict with the new TcwGBA, Tcw, TcwBefGBA (rows of reached keyframes, zero elsewhere), kf_done, pos,
    n_kf_propagated, n_mp_gba, n_mp_moved, depth.  A keyframe is visited once (the relation is a tree)."""
    T, G = _rows16(Tcw), _rows16(TcwGBA)
    in_gba = [bool(v) for v in kf_in_gba]
    pos = np.array(pos, np.float32).reshape(-1, 3)
    Bef = [[0.0] * 16 for _ in T]
    done = [False] * len(T)
    chain = [0] * len(T)
    n_prop = 0
    lpKFtoCheck = []
    for o in origins:
        o = int(o)
        if ref.live(o) is not None and not done[o]:
            done[o] = True
            lpKFtoCheck.append(o)
    while lpKFtoCheck:
        k = lpKFtoCheck[0]
        Twc = twc(T[k])                                  # pKF->GetPoseInverse()
        for c in ref.kfs[k].children:
            if ref.live(c) is None or done[c]:
                continue
            done[c] = True
            if not in_gba[c]:
                G[c] = gemm(gemm(T[c], Twc), G[k])       # Tchildc * pKF->mTcwGBA
                in_gba[c] = True
                chain[c] = chain[k] + 1
                n_prop += 1
            lpKFtoCheck.append(c)
        Bef[k] = T[k]
        T[k] = G[k]                                      # pKF->SetPose(pKF->mTcwGBA)
        lpKFtoCheck.pop(0)
    n_gba = n_moved = 0
    for p in range(len(pos)):
        if bad is not None and bad[p]:
            continue
        if mp_in_gba[p]:
            pos[p] = np.asarray(posGBA, np.float32).reshape(-1, 3)[p]
            n_gba += 1
            continue
        r = int(ref_kf[p])
        if r < 0 or r >= len(T) or not done[r]:
            continue
        Xc = rot_apply(Bef[r], [float(v) for v in pos[p]])     # Rcw * pos + tcw of mTcwBefGBA
        pos[p] = rot_apply(twc(T[r]), Xc)                      # Rwc * Xc + twc of GetPoseInverse()
        n_moved += 1
    return dict(TcwGBA=np.array(G, np.float32), Tcw=np.array(T, np.float32), TcwBefGBA=np.array(Bef, np.float32),
                kf_done=np.array(done, np.uint8), pos=pos, n_kf_propagated=n_prop, n_mp_gba=n_gba,
                n_mp_moved=n_moved, depth=max(chain) if chain else 0)


# ---- float64 models -----------------------------------------------------------------------------
def _sim3_mat(S):
    """A Sim3 as the 4 x 4 [sR | t] with R from the normalised quaternion."""
    q = np.asarray(S[:4], np.float64)
    x, y, z, w = q / np.linalg.norm(q)
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    M = np.eye(4)
    M[:3, :3] = float(S[7]) * R
    M[:3, 3] = S[4:7]
    return M


def ref64_correct_loop(ref, kf, cur_kf, Scw, Tcw, pos, bad=None):
    """Positions and poses only, in float64: -> (Tcw n x 4 x 4, pos n x 3, corrected_ref dict)."""
    T = np.asarray(Tcw, np.float64).reshape(-1, 4, 4).copy()
    old = T.copy()
    pos = np.asarray(pos, np.float64).reshape(-1, 3).copy()
    S = _sim3_mat(Scw)
    who = {}
    for i in sorted(int(k) for k in kf):
        Ci = S if i == cur_kf else old[i] @ np.linalg.inv(old[cur_kf]) @ S
        for pMP in ref.kfs[i].mvpMapPoints:
            if pMP is None or pMP.isBad() or pMP.mnId >= len(pos) or pMP.mnId in who:
                continue
            if bad is not None and bad[pMP.mnId]:
                continue
            who[pMP.mnId] = i
            pos[pMP.mnId] = (np.linalg.inv(Ci) @ old[i] @ np.append(pos[pMP.mnId], 1.0))[:3]
        s = np.cbrt(np.linalg.det(Ci[:3, :3]))
        T[i] = np.eye(4)
        T[i][:3, :3] = Ci[:3, :3] / s
        T[i][:3, 3] = Ci[:3, 3] / s
    return T, pos, who


def ref64_apply_gba(ref, origins, TcwGBA, kf_in_gba, Tcw, pos, posGBA, mp_in_gba, ref_kf, bad=None):
    """-> (Tcw n x 4 x 4, pos n x 3) in float64."""
    old = np.asarray(Tcw, np.float64).reshape(-1, 4, 4)
    G = np.asarray(TcwGBA, np.float64).reshape(-1, 4, 4).copy()
    T = old.copy()
    pos = np.asarray(pos, np.float64).reshape(-1, 3).copy()
    done = set()
    queue = [int(o) for o in origins if ref.live(int(o)) is not None]
    done.update(queue)
    in_gba = [bool(v) for v in kf_in_gba]
    while queue:
        k = queue.pop(0)
        for c in ref.kfs[k].children:
            if ref.live(c) is None or c in done:
                continue
            done.add(c)
            if not in_gba[c]:
                G[c] = old[c] @ np.linalg.inv(old[k]) @ G[k]
            queue.append(c)
        T[k] = G[k]
    for p in range(len(pos)):
        if bad is not None and bad[p]:
            continue
        if mp_in_gba[p]:
            pos[p] = np.asarray(posGBA, np.float64).reshape(-1, 3)[p]
        elif 0 <= int(ref_kf[p]) < len(T) and int(ref_kf[p]) in done:
            r = int(ref_kf[p])
            pos[p] = (np.linalg.inv(T[r]) @ old[r] @ np.append(pos[p], 1.0))[:3]
    return T, pos
