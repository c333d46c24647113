"""Seeded inputs for LoopClosing_SearchAndFuse, built on the maps of tests/fuse_cases.py.  The FuseCase's
current keyframe plays the loop side: mvpLoopMapPoints is its row.  Its other real keyframes are the listed
(corrected) ones; the Sim3 of a keyframe with pose (R, t) is (q(R), s t, s) with s cycling over 1, 0.93, 1.08,
0.97, so Rcw = R and tcw = t up to rounding, the projections still land on the keypoints and the
normalisation by scw is exercised.  mpCurrentKF is the listed keyframe of highest id: mvpCurrentMatchedPoints
names, for a seeded half of its held slots, the loop point with the same position bytes (the slot's own
point: Replace returns at once; a duplicate: a Replace) and, for about 5 % of its empty slots, a loop point
that is not in the row (an AddMapPoint).

A case hands the same map to the library's Map and to the reference's CullRefMap."""
import functools

import numpy as np

from fuse_cases import LOG_SF, FuseCase

SCALES = (1.0, 0.93, 1.08, 0.97)
TH = 4.0


def quat_of(R):
    """A unit quaternion (x, y, z, w) of the rotation matrix R, in float64."""
    R = np.asarray(R, np.float64)
    w = np.sqrt(max(0.0, 1.0 + R[0, 0] + R[1, 1] + R[2, 2])) / 2.0
    assert w > 0.25, "the cases' rotations are small"
    q = np.array([(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w])
    return q / np.linalg.norm(q)


class LoopFuseCase:
    def __init__(self, base, seed, listed=None, with_loop=True, with_matched=True, held_twice=False):
        rng = np.random.default_rng(7000 + seed)
        self.base = base
        rows = {op[1]: op[2] for op in base.ops if op[0] == "AddKeyFrame"}
        others = sorted(k for k in base.real_ids if k != base.cur_kf)
        ids = others if listed is None else [others[j] for j in listed]
        self.scw_of = {}
        for j, kid in enumerate(sorted(ids)):
            T = base.frames[kid].Tcw.astype(np.float64)
            s = SCALES[j % len(SCALES)]
            self.scw_of[kid] = np.concatenate([quat_of(T[:3, :3]), s * T[:3, 3], [s]])
        self.kf = [ids[j] for j in rng.permutation(len(ids))]          # the caller's order is not the pass order
        self.loop_pts = rows[base.cur_kf].copy() if with_loop else np.zeros(0, np.int32)
        self.kf_desc, self.n_kf_rows, self.n_pts = base.kf_desc, base.n_kf_rows, base.n_pts
        self.table = {k: base.table[k] for k in ("pos", "normal", "max_dist", "min_dist", "desc", "bad")}
        self.cur_kf, self.matched = -1, None
        if with_matched and ids:
            self.cur_kf = max(ids)
            self.matched = self._held_twice(rows, rng) if held_twice else self._matched(rows, rng)
            self.matched.setflags(write=False)       # cases are shared between tests
        self.loop_pts.setflags(write=False)

    def _loop_by_pos(self):
        bad, pos = self.table["bad"], self.table["pos"]
        at = {}
        for L in self.loop_pts:
            if L >= 0 and not bad[L]:
                at.setdefault(pos[L].tobytes(), int(L))
        return at

    def _matched(self, rows, rng):
        row = rows[self.cur_kf]
        at = self._loop_by_pos()
        matched = np.full(len(row), -1, np.int32)
        used = set()
        for i in np.flatnonzero(row >= 0):
            L = at.get(self.table["pos"][row[i]].tobytes())
            if L is not None and rng.random() < 0.5:
                matched[i] = L
                used.add(L)
        inrow = set(int(p) for p in row if p >= 0)
        pool = [L for L in at.values() if L not in inrow and L not in used]
        pool = [pool[j] for j in rng.permutation(len(pool))]
        for i in np.flatnonzero(row < 0):
            if pool and rng.random() < 0.05:
                matched[i] = pool.pop()
        return matched

    def _held_twice(self, rows, rng):
        """A loop point L that slot j of the row holds, named by a held slot (its point is replaced by L: the
        slot empties) and by an empty slot (skipped: n_matched_skipped)."""
        row = rows[self.cur_kf]
        loop = set(int(p) for p in self.loop_pts if p >= 0 and not self.table["bad"][p])
        j = next(int(i) for i in np.flatnonzero(row >= 0) if int(row[i]) in loop)
        L = int(row[j])
        held = next(int(i) for i in np.flatnonzero(row >= 0) if i != j and not self.table["bad"][row[i]])
        empty = int(np.flatnonzero(row < 0)[0])
        matched = np.full(len(row), -1, np.int32)
        matched[held] = matched[empty] = L
        self.twice = dict(L=L, at=j, held=held, empty=empty, replaced=int(row[held]))
        return matched

    @property
    def frames(self):
        return [self.base.frames[k] for k in self.kf]

    @property
    def Scw(self):
        return np.array([self.scw_of[k] for k in self.kf], np.float64).reshape(-1, 8)

    def fill(self, target):
        return self.base.fill(target)

    def refmap(self):
        return self.base.refmap()

    def table_copy(self):
        return {k: v.copy() for k, v in self.table.items()}

    def kwargs(self, table, order=None):
        """keyword arguments of LoopClosing.SearchAndFuse / of the reference; order: a permutation of kf[]"""
        o = list(range(len(self.kf))) if order is None else list(order)
        return dict(kf=[self.kf[j] for j in o], frames=[self.frames[j] for j in o], Scw=self.Scw[o].reshape(-1, 8),
                    loop_pts=self.loop_pts, kf_desc=self.kf_desc, table=table, logScaleFactor=LOG_SF, cur_kf=self.cur_kf,
                    matched=self.matched, th=TH, n_kf_rows=self.n_kf_rows)


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "mono":
        return LoopFuseCase(FuseCase(0, 0.0), 0)
    if name == "stereo":
        return LoopFuseCase(FuseCase(1, 0.5), 1)
    if name == "twice":
        return LoopFuseCase(FuseCase(2, 0.5, n_real=4, targets=[0, 1, 2, 0]), 2)
    if name == "no_keyframes":
        return LoopFuseCase(FuseCase(0, 0.0), 3, listed=[])
    if name == "empty_loop":
        return LoopFuseCase(FuseCase(0, 0.0), 4, with_loop=False)
    if name == "no_matched":
        return LoopFuseCase(FuseCase(1, 0.5), 5, with_matched=False)
    if name == "one_keyframe":
        return LoopFuseCase(FuseCase(4, 0.5, targets=[1]), 6, listed=[1])
    if name == "matched_held_twice":
        return LoopFuseCase(FuseCase(4, 0.5, targets=[1]), 7, listed=[1], held_twice=True)
    raise KeyError(name)


MAIN = ["mono", "stereo", "twice"]
EDGE = ["no_keyframes", "empty_loop", "no_matched", "one_keyframe", "matched_held_twice"]
