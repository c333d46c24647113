"""Seeded case builders for the LoopClosing map-correction tests: a map (mutation ops for the library's Map
and the RefMap alike, per-slot octaves), the keyframe pose table, the map-point table and the call's
arguments.  Shared by the CPU test of the restatement and the GPU test of the library."""
import numpy as np

import loopcorrect_ref as lr
from map_ref import RefMap

NLEVELS = 8
SCALE_FACTORS = np.array([1.2 ** k for k in range(NLEVELS)], np.float32)


def rodrigues(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def random_pose(rng, k):
    """A float32 Tcw.  Every fourth pose is rotated close to 180 degrees about x, y or z (the three
    trace <= 0 branches of the quaternion conversion); the others by less than 90 degrees."""
    if k % 4 == 3:
        axis = np.eye(3)[(k // 4) % 3] + rng.normal(0, 0.02, 3)
        R = rodrigues(axis, np.pi - rng.uniform(0.0, 0.05))
    else:
        R = rodrigues(rng.normal(0, 1, 3), rng.uniform(0.0, 1.4))
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = rng.uniform(-5, 5, 3)
    return T.astype(np.float32)


def sim3_near(rng, Tcw, s):
    """mg2oScw: the pose of the current keyframe moved a little, with scale s."""
    R = rodrigues(rng.normal(0, 1, 3), rng.uniform(0.01, 0.1)) @ np.asarray(Tcw, np.float64)[:3, :3]
    q = lr.quat_from_R([float(v) for v in R.ravel()])
    t = np.asarray(Tcw, np.float64)[:3, 3] + rng.normal(0, 0.2, 3)
    return np.array(q + [float(v) for v in t] + [float(s)], np.float64)


def apply(target, ops):
    for op in ops:
        getattr(target, op[0])(*op[1:])


class CorrectCase:
    """rows[i] = the slot count of keyframe i (ids 0 .. len(rows) - 1); listed = the ids passed as kf."""

    def __init__(self, seed, rows, listed, n_pts, s=1.0, identity=False, hot=True):
        rng = np.random.default_rng(seed)
        n_kf = len(rows)
        self.n_pts, self.n_kf_rows = n_pts, n_kf + 2
        self.kf = np.array(listed, np.int32)
        self.cur_kf = int(listed[len(listed) // 2])
        self.ops, self.octaves = [], {}
        # point 0 is observed by every listed keyframe that has a slot, and by no other; point 1 is
        # held by the first listed keyframes in unobserved slots only (no observers); point 2 has at most
        # one observer and point 3 at most three, among the listed keyframes
        listed_rows = [k for k in listed if rows[k] > 0]
        for k in range(n_kf):
            N = rows[k]
            mp = np.full(N, -1, np.int32)
            obs = (rng.random(N) >= 0.1).astype(np.uint8)
            free = list(rng.permutation(N))
            special = []
            if hot and k in listed_rows:
                special.append((0, 1))
            if k in listed_rows[:2]:
                special.append((1, 0))
            if k in listed_rows[-1:]:
                special.append((2, 1))
            if k in listed_rows[:3]:
                special.append((3, 1))
            for p, o in special:
                if free:
                    i = free.pop()
                    mp[i], obs[i] = p, o
            take = rng.permutation(np.arange(4, n_pts))[:min(int(0.8 * len(free)), max(n_pts - 4, 0))]
            for p in take:
                mp[free.pop()] = p
            self.ops.append(("AddKeyFrame", k, mp, obs))
            self.octaves[k] = rng.integers(0, NLEVELS, N).astype(np.uint8)
        self.Tcw = np.zeros((self.n_kf_rows, 16), np.float32)
        for k in range(n_kf):
            self.Tcw[k] = random_pose(rng, k + seed).ravel()
        if identity:
            self.Scw = np.array(lr.sim3_of_pose([float(v) for v in self.Tcw[self.cur_kf]]), np.float64)
        else:
            self.Scw = sim3_near(rng, self.Tcw[self.cur_kf].reshape(4, 4), s)
        self.pos = rng.uniform(-10, 10, (n_pts, 3)).astype(np.float32)
        self.normal = rng.normal(0, 1, (n_pts, 3)).astype(np.float32)
        self.max_dist = rng.uniform(5, 20, n_pts).astype(np.float32)
        self.min_dist = rng.uniform(0.1, 2, n_pts).astype(np.float32)
        self.corrected_ref = np.full(n_pts, -7, np.int32)
        self.bad = (rng.random(n_pts) < 0.05).astype(np.uint8)
        self.bad[:4] = 0
        ref = self.refmap()
        self.ref_kf = np.full(n_pts, -1, np.int32)
        for p, m in ref.pts.items():
            if p >= n_pts:
                continue
            ids = sorted(k.mnId for k in m.mObservations)
            u = rng.random()
            if ids and u < 0.85:
                self.ref_kf[p] = ids[int(rng.integers(0, len(ids)))]
            elif u < 0.92:
                self.ref_kf[p] = int(rng.integers(0, n_kf))      # usually not an observer
        # a bad point whose only holders are listed keyframes
        for p, m in ref.pts.items():
            if 4 <= p < n_pts and m.mObservations and all(k.mnId in listed for k in m.mObservations):
                self.bad[p] = 1
                break

    def refmap(self, extra_ops=()):
        ref = RefMap()
        apply(ref, self.ops)
        apply(ref, extra_ops)
        return ref

    def tables(self):
        return dict(Tcw=self.Tcw.copy(), pos=self.pos.copy(), normal=self.normal.copy(),
                    max_dist=self.max_dist.copy(), min_dist=self.min_dist.copy(), ref_kf=self.ref_kf.copy(),
                    corrected_ref=self.corrected_ref.copy(), bad=self.bad.copy())

    def restate(self, ref=None, kf=None, bad=None):
        t = self.tables()
        return lr.restate_correct_loop(ref or self.refmap(), self.octaves, self.kf if kf is None else kf, self.cur_kf,
                                       self.Scw, SCALE_FACTORS, t["Tcw"], t["pos"], t["normal"], t["max_dist"],
                                       t["min_dist"], t["ref_kf"], t["corrected_ref"], t["bad"] if bad is None else bad)


def correct_cases():
    """name -> CorrectCase: 1, 2, 3 and 70 listed keyframes; rows of 0, 1, 65, 300 and 4096 slots; points with
    0, 1, 3 and more than 70 observers; scales 1, 0.5 and 3."""
    return {
        "one_listed": CorrectCase(1, [65, 65, 65], [1], 120, s=1.0),
        "two_listed_tiny_rows": CorrectCase(2, [1, 0, 1, 65], [3, 0, 1], 40, s=0.5, hot=False),
        "two_listed": CorrectCase(3, [65, 300, 65], [2, 0], 400, s=3.0),
        "three_listed_wide": CorrectCase(4, [0, 1, 65, 300, 4096, 65], [4, 1, 3], 6000, s=0.5),
        "seventy_listed": CorrectCase(5, [300] * 80, list(range(3, 73)), 3000, s=3.0),
        "identity": CorrectCase(6, [65] * 6, [0, 2, 3, 5], 200, identity=True),
    }


class GbaCase:
    """nodes: (id, parent or -1, in_gba); origins; dead: ids named as children that were never in the map;
    erase: keyframes erased after the tree is set (their subtrees are cut off)."""

    def __init__(self, seed, nodes, origins, n_pts, dead=(), erase=(), n_extra_rows=2):
        rng = np.random.default_rng(seed)
        ids = [n[0] for n in nodes]
        self.origins = np.array(origins, np.int32)
        self.n_kf_rows = max(ids) + 1 + n_extra_rows
        self.n_pts = n_pts
        children = {k: [] for k in ids}
        for k, par, _ in nodes:
            if par >= 0:
                children[par].append(k)
        for i, d in enumerate(dead):
            children[ids[i % len(ids)]].append(int(d))
        self.ops = [("AddKeyFrame", k, np.zeros(0, np.int32), None) for k in ids]
        self.ops += [("SetNeighbours", k, np.zeros(0, np.int32), par, np.array(children[k], np.int32))
                     for k, par, _ in nodes]
        self.ops += [("EraseKeyFrame", int(k)) for k in erase]
        self.kf_in_gba = np.zeros(self.n_kf_rows, np.uint8)
        self.Tcw = np.zeros((self.n_kf_rows, 16), np.float32)
        self.TcwGBA = np.zeros((self.n_kf_rows, 16), np.float32)
        for k, _, g in nodes:
            self.kf_in_gba[k] = g
            self.Tcw[k] = random_pose(rng, k + seed).ravel()
            if g:   # the optimised pose: the old one moved a little
                T = self.Tcw[k].reshape(4, 4).astype(np.float64)
                D = np.eye(4)
                D[:3, :3] = rodrigues(rng.normal(0, 1, 3), rng.uniform(0.0, 0.05))
                D[:3, 3] = rng.normal(0, 0.1, 3)
                self.TcwGBA[k] = (D @ T).astype(np.float32).ravel()
        self.pos = rng.uniform(-10, 10, (n_pts, 3)).astype(np.float32)
        self.posGBA = (self.pos + rng.normal(0, 0.05, (n_pts, 3))).astype(np.float32)
        self.mp_in_gba = (rng.random(n_pts) < 0.4).astype(np.uint8)
        self.bad = (rng.random(n_pts) < 0.1).astype(np.uint8)
        # references: any row of the table (reached, unreached or never used) or -1
        self.ref_kf = rng.integers(-1, self.n_kf_rows, n_pts).astype(np.int32)

    def refmap(self):
        ref = RefMap()
        apply(ref, self.ops)
        return ref

    def restate(self):
        return lr.restate_apply_gba(self.refmap(), self.origins, self.TcwGBA, self.kf_in_gba, self.Tcw, self.pos,
                                    self.posGBA, self.mp_in_gba, self.ref_kf, self.bad)


def _chain(first_id, parent, length, in_gba=0):
    return [(first_id + i, parent if i == 0 else first_id + i - 1, in_gba) for i in range(length)]


def gba_cases():
    """name -> GbaCase.  Point counts 0, 1, 257 and 5,000 are spread over the trees."""
    rng = np.random.default_rng(11)
    tree = [(0, -1, 1)] + [(k, int(rng.integers(0, k)), 1) for k in range(1, 20)]
    mixed = [(0, -1, 1), (1, 0, 1), (2, 1, 0), (3, 0, 1)]            # depth 1 below an optimised keyframe
    mixed += _chain(4, 3, 5) + [(9, 6, 1)] + _chain(10, 9, 2)        # depth 5, an optimised one inside, depth 2
    return {
        "origin_alone": GbaCase(1, [(0, -1, 1)], [0], 1),
        "all_in_ba": GbaCase(2, tree, [0], 257),
        "mixed_depths": GbaCase(3, mixed, [0], 257),
        "chain_70": GbaCase(4, [(0, -1, 1), (1, 0, 1)] + _chain(2, 1, 70), [0], 0),
        "fan_300": GbaCase(5, [(0, -1, 1)] + [(k, 0, 0) for k in range(1, 301)], [0], 5000),
        "two_origins": GbaCase(6, [(0, -1, 1), (1, 0, 0), (2, -1, 1), (3, 2, 0), (4, 3, 0)], [2, 0], 257),
        "unreached": GbaCase(7, [(0, -1, 1), (1, 0, 0), (5, -1, 1), (6, 5, 0)], [0], 257),
        "dead_child": GbaCase(8, [(0, -1, 1), (1, 0, 0), (2, 1, 0), (3, 1, 0), (4, 3, 0)], [0], 257, dead=(40, 41),
                              erase=(3,)),
    }
