"""Seeded inputs for LocalMapping::SearchInNeighbors: a handful of real keyframes (oracle extraction of
synthetic.sequence frames, the current keyframe in the middle), map points lifted from the current keyframe's
keypoints, and per target keyframe, for the same physical feature and at seeded rates, the shared id (the
pass skips it), a distinct id (a duplicate: a Replace) or no point (an AddObservation).  "Ghost" keyframes
exist only in the relation, in kf_desc and in Ow: they vary Observations(), so both Replace directions
occur, and they carry chosen descriptors, so the distinctive descriptor of a merged point moves.

A case hands the same mutations to the library's Map and to the reference's CullRefMap."""
import functools

import numpy as np

import oracle_lib
from c_orb_slam_amd import synthetic
from c_orb_slam_amd.orb import Frame
from culling_ref import CullRefMap

W, H = 1241, 376
LOG_SF = np.float32(np.log(np.float32(1.2)))
_POP = np.array([bin(i).count("1") for i in range(256)], np.uint8)


@functools.lru_cache(maxsize=None)
def _frames(seed, n):
    imgs, _, Rs = synthetic.sequence(seed, n, W, H, return_rotations=True)
    ex = oracle_lib.OracleExtractor(600, 1.2, 8, 20, 7)
    return [ex(im) for im in imgs], Rs, ex.tables()


def _flip(rng, d, nbits):
    out = d.copy()
    for b in rng.choice(256, nbits, replace=False):
        out[b >> 3] ^= np.uint8(1 << (b & 7))
    return out


class FuseCase:
    def __init__(self, seed, stereo_frac=0.0, n_real=5, targets=None, empty_cur=False, n_ghost=8):
        rng = np.random.default_rng(1000 + seed)
        (kd, Rs, tab) = _frames(seed, n_real)
        self.scale = tab["scale"]
        nl = len(self.scale)
        K4 = synthetic.intrinsics(W, H)
        fx, fy, cx, cy = K4
        c = n_real // 2
        real_ids = [3, 5, 6, 8, 9][:n_real]
        self.cur_kf = real_ids[c]
        ghost_ids = [0, 1, 4, 7, 11, 12, 14, 15][:n_ghost]
        self.n_kf_rows = 18
        # poses: world = the current keyframe's camera; rotations of the sequence, millimetres of translation
        A = [None] * n_real
        A[c] = np.eye(3)
        for k in range(c, n_real - 1):
            A[k + 1] = Rs[k] @ A[k]
        for k in range(c - 1, -1, -1):
            A[k] = Rs[k].T @ A[k + 1]
        T = []
        for k in range(n_real):
            t = np.zeros(3) if k == c else rng.normal(0, 1e-3, 3)
            T.append(synthetic.pose_from_rotation(A[k], t))
        Ow = rng.normal(0, 2.0, (self.n_kf_rows, 3)).astype(np.float32)      # the ghosts' centres are anywhere
        for k in range(n_real):
            Ow[real_ids[k]] = (-(T[k][:3, :3].astype(np.float64).T @ T[k][:3, 3].astype(np.float64))).astype(np.float32)
        self.Ow = Ow

        kc, dc = kd[c]
        nc = len(kc)
        X = synthetic.lift_map_points(rng, kc, K4)                           # cur camera = world
        # the map-point table grows as duplicates are made
        pos, desc, normal, maxd, mind, ref_kf = [], [], [], [], [], []

        def new_point(Xw, d, centre, octave, ref):
            PC = Xw.astype(np.float32) - centre
            dist = np.float32(np.linalg.norm(PC))
            pos.append(Xw.astype(np.float32))
            desc.append(d.copy())
            normal.append((PC / dist).astype(np.float32))
            maxd.append(np.float32(dist * self.scale[octave]))
            mind.append(np.float32(maxd[-1] / self.scale[-1]))
            ref_kf.append(ref)
            return len(pos) - 1

        for i in range(nc):
            new_point(X[i], dc[i], Ow[self.cur_kf], int(kc["octave"][i]), self.cur_kf)
        rows = {real_ids[k]: np.full(len(kd[k][0]), -1, np.int32) for k in range(n_real)}
        held = rng.random(nc) < (0.0 if empty_cur else 0.8)
        rows[self.cur_kf][:] = np.where(held, np.arange(nc), -1)
        # twins: a second point of the same physical feature in a free slot of the current row, so that two
        # points of one pass choose the same keypoint
        free = list(np.flatnonzero(~held))
        twins = []
        if not empty_cur:
            for i in rng.permutation(np.flatnonzero(held))[:12]:
                if not free:
                    break
                p = new_point(X[i], dc[i], Ow[self.cur_kf], int(kc["octave"][i]), self.cur_kf)
                rows[self.cur_kf][free.pop()] = p
                twins.append(p)
        uR = {}
        dups = []
        for k in range(n_real):
            if k == c:
                continue
            kk, dk = kd[k]
            Tk = T[k].astype(np.float64)
            Xc = X.astype(np.float64) @ Tk[:3, :3].T + Tk[:3, 3]
            u, v = fx * Xc[:, 0] / Xc[:, 2] + cx, fy * Xc[:, 1] / Xc[:, 2] + cy
            d2 = (kk["x"][None, :] - u[:, None]) ** 2 + (kk["y"][None, :] - v[:, None]) ** 2
            near = d2.argmin(axis=1)
            ur = np.where(rng.random(len(kk)) < stereo_frac, kk["x"] - rng.uniform(2, 40, len(kk)), -1.0).astype(np.float32)
            used = set()
            for i in range(nc):
                j = int(near[i])
                ham = int(_POP[dc[i] ^ dk[j]].sum())
                if d2[i, j] > 1.5 ** 2 or kk["octave"][j] != kc["octave"][i] or ham > 45 or j in used:
                    continue
                used.add(j)
                if ur[j] >= 0:                                       # a stereo keypoint agrees with the point's depth
                    ur[j] = np.float32(kk["x"][j] - synthetic.KITTI_BF / Xc[i, 2])
                r = rng.random()
                if held[i] and r < 0.25:
                    rows[real_ids[k]][j] = i                                 # the shared id
                elif r < 0.60:
                    p = new_point(X[i], dk[j], Ow[real_ids[k]], int(kk["octave"][j]), real_ids[k])
                    rows[real_ids[k]][j] = p                                 # a duplicate
                    dups.append(p)
                # else: no point at that keypoint
            uR[real_ids[k]] = ur if stereo_frac > 0 else None
        uR[self.cur_kf] = None
        self.frames = {real_ids[k]: Frame(kd[k][0], kd[k][1], self.scale, T[k], fx, fy, cx, cy, synthetic.KITTI_BF, W, H,
                                          uRight=uR[real_ids[k]]) for k in range(n_real)}
        n = len(pos)
        # ghosts: extra observers with their own descriptor rows
        moved = set(int(i) for i in rng.permutation(nc)[:nc // 6] if held[i])
        ghost_rows = {g: [] for g in ghost_ids}                              # (point, descriptor, octave, stereo)
        for p in range(n):
            base = np.asarray(desc[p])
            if p in moved:
                far = _flip(rng, base, 90)
                for g in rng.permutation(ghost_ids)[:4]:
                    ghost_rows[int(g)].append((p, far, int(rng.integers(0, nl)), rng.random() < 0.3))
            else:
                for g in rng.permutation(ghost_ids)[:int(rng.integers(0, 4))]:
                    ghost_rows[int(g)].append((p, _flip(rng, base, int(rng.integers(0, 8))), int(rng.integers(0, nl)),
                                               rng.random() < 0.3))
        self.kf_desc = {kid: self.frames[kid].desc for kid in real_ids}
        self.ops = []
        for kid in real_ids:
            F = self.frames[kid]
            self.ops.append(("AddKeyFrame", kid, rows[kid].copy()))
            self.ops.append(("SetKeyFrameKeys", kid, F.keysUn["octave"].astype(np.uint8), F.uRight))
        for g in ghost_ids:
            gr = ghost_rows[g]
            self.kf_desc[g] = np.stack([r[1] for r in gr]) if gr else np.zeros((0, 32), np.uint8)
            self.ops.append(("AddKeyFrame", g, np.array([r[0] for r in gr], np.int32)))
            self.ops.append(("SetKeyFrameKeys", g, np.array([r[2] for r in gr], np.uint8),
                             np.array([1.0 if r[3] else -1.0 for r in gr], np.float32)))
        bad = np.zeros(n, np.uint8)
        for p in rng.permutation(dups)[:max(2, len(dups) // 40)]:
            bad[p] = 1                                                       # bad in the table, still held
        for i in rng.permutation(np.flatnonzero(held))[:5]:
            bad[i] = 1
        ref = np.array(ref_kf, np.int32)
        cur_pts = np.flatnonzero(held)
        for i in rng.permutation(cur_pts)[:6]:
            ref[i] = -1                                                      # no reference keyframe
        for i in rng.permutation(cur_pts)[:6]:
            ref[i] = 16                                                      # an id nobody has
        self.table = dict(pos=np.array(pos, np.float32).reshape(-1, 3), desc=np.array(desc, np.uint8).reshape(-1, 32),
                          normal=np.array(normal, np.float32).reshape(-1, 3), max_dist=np.array(maxd, np.float32),
                          min_dist=np.array(mind, np.float32), bad=bad, ref_kf=ref)
        others = [kid for kid in real_ids if kid != self.cur_kf]
        order = [others[j] for j in rng.permutation(len(others))]
        self.target_ids = order if targets is None else [others[j] for j in targets]
        self.real_ids, self.ghost_ids, self.n_pts, self.twins, self.dups = real_ids, ghost_ids, n, twins, dups

    @property
    def targets(self):
        return [self.frames[k] for k in self.target_ids]

    @property
    def cur(self):
        return self.frames[self.cur_kf]

    def fill(self, target):
        """Hand the case's map to a c_orb_slam_amd.Map or a CullRefMap."""
        for op in self.ops:
            getattr(target, op[0])(*op[1:])
        return target

    def refmap(self):
        return self.fill(CullRefMap())

    def table_copy(self):
        return {k: v.copy() for k, v in self.table.items()}

    def args(self, table):
        """positional arguments after the matcher for Map.SearchInNeighbors / after the RefMap for the reference"""
        return (self.cur_kf, self.cur, self.target_ids, self.targets, self.kf_desc, self.Ow, self.scale, table, LOG_SF)


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "mono":
        return FuseCase(0, 0.0)
    if name == "stereo":
        return FuseCase(1, 0.5)
    if name == "twice":                 # the first target comes back after the others
        return FuseCase(2, 0.5, n_real=4, targets=[0, 1, 2, 0])
    if name == "no_targets":
        return FuseCase(0, 0.0, targets=[])
    if name == "empty_cur":
        return FuseCase(3, 0.0, empty_cur=True)
    if name == "one_target":
        return FuseCase(4, 0.5, targets=[1])
    raise KeyError(name)


MAIN = ["mono", "stereo", "twice"]
EDGE = ["no_targets", "empty_cur", "one_target"]
