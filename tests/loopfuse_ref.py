"""A literal restatement of the loop fusion of LoopClosing::CorrectLoop (src/LoopClosing.cc): the "Start
Loop Fusion" block over mvpCurrentMatchedPoints and LoopClosing::SearchAndFuse, from the parts the suite
already has: the relation and MapPoint::Replace of culling_ref.CullRefMap, the per-pass selection of
ORBmatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) (src/ORBmatcher.cc:977-1100) by the CPU oracle, and
ComputeDistinctiveDescriptors as localmap_ref restates it.

Everything runs where the reference runs it: AddObservation / AddMapPoint inside the loop over the points,
the Replaces after each Fuse, ComputeDistinctiveDescriptors inside Replace.  The oracle is asked once per
pass with the skip flags of the pass's start; what that rests on is asserted, not assumed.

plan_first=True is the wrong adapter this entry exists to replace: every pass matches with the descriptors
and bad flags the call started with.  Nothing here is shared with the library."""
import numpy as np

import oracle_lib
from c_orb_slam_amd.orb import MapPointGeo, MapPoints
from localmap_ref import restate_best


def cvScw_of(S8):
    """Converter::toCvMat(g2o::Sim3): R = q.toRotationMatrix() (Eigen's formula) in float64, then the float
    matrix [s R | t; 0 0 0 1]."""
    x, y, z, w, s = (np.float64(v) for v in (S8[0], S8[1], S8[2], S8[3], S8[7]))
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    R = np.array([[1.0 - (tyy + tzz), txy - twz, txz + twy],
                  [txy + twz, 1.0 - (txx + tzz), tyz - twx],
                  [txz - twy, tyz + twx, 1.0 - (txx + tyy)]], np.float64)
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = (s * R).astype(np.float32)
    T[:3, 3] = np.asarray(S8[4:7], np.float64).astype(np.float32)
    return T


class SearchAndFuseRef:
    def __init__(self, ref, kf, frames, Scw, loop_pts, kf_desc, table, logScaleFactor, cur_kf=-1, matched=None,
                 th=4.0, n_kf_rows=None, plan_first=False):
        """ref: a culling_ref.CullRefMap (changed as the reference changes the map); table: dict of arrays,
        copied here.  The results are the attributes t (the table), ops, nfused, updated, n_matched_skipped."""
        self.ref = ref
        self.kf, self.frames = [int(k) for k in kf], list(frames)
        self.Scw = np.asarray(Scw, np.float64).reshape(-1, 8)
        self.loop_pts = [int(p) for p in loop_pts]
        self.kf_desc = kf_desc
        self.t = {k: np.array(v, copy=True) for k, v in table.items()}
        self.start_desc, self.start_bad = self.t["desc"].copy(), self.t["bad"].copy()
        self.lsf, self.th, self.plan_first = np.float32(logScaleFactor), float(th), plan_first
        self.cur_kf, self.matched = int(cur_kf), None if matched is None else [int(m) for m in matched]
        self.ops, self.nfused, self.updated, self.n_matched_skipped = [], [0] * len(self.kf), set(), 0
        # what the cases are required to reach (tests/test_loopfuse_cases_cpu.py)
        self.same_keypoint = 0       # points choosing a keypoint another point of the pass took
        self.dead_replaced = 0       # Replaces of a point an earlier Replace already made bad
        self.loop_by_loop = 0        # loop points replaced by another loop point
        self.step0_same = 0          # step 0 entries whose slot already holds L
        self.desc_changed = set()    # survivors whose descriptor row changed

    # ---- MapPoint
    def isBad(self, p):
        return bool(self.t["bad"][p])

    def _observations(self, p):
        """mObservations in ascending keyframe id: [(KeyFrame, idx)]"""
        return sorted(self.ref.point(p).mObservations.items(), key=lambda kv: kv[0].mnId)

    def ComputeDistinctiveDescriptors(self, p):
        if self.isBad(p):
            return
        obs = self._observations(p)
        if not obs:
            return
        rows = np.stack([self.kf_desc[kf.mnId][idx] for kf, idx in obs])
        new = rows[restate_best(rows)]
        if not np.array_equal(new, self.t["desc"][p]):
            self.desc_changed.add(p)
        self.t["desc"][p] = new
        self.updated.add(p)
        self.recomputed[p] = new.copy()

    def Replace(self, a, b, where):
        """a->Replace(b) (MapPoint.cc): Map_ReplaceMapPoint's relation change, the flag, the descriptor"""
        if a == b:
            return
        if a in self.replaced:                       # replaced again: it is bad and nobody observes it
            assert self.plan_first or (self.isBad(a) and not self.ref.point(a).mObservations)
            self.dead_replaced += 1
        self.ref.ReplaceMapPoint(a, b)
        self.t["bad"][a] = 1
        self.replaced.add(a)
        self.updated.add(a)
        self.ops.append((where[0], 2, a, b, where[1], where[2]))
        self.ComputeDistinctiveDescriptors(b)

    # ---- the "Start Loop Fusion" block of CorrectLoop
    def step0(self):
        pCur = self.ref.kfs[self.cur_kf]
        assert len(self.matched) == len(pCur.mvpMapPoints)
        self.recomputed = {}
        for i, L in enumerate(self.matched):
            if L < 0:
                continue
            pCurMP = pCur.mvpMapPoints[i]
            if pCurMP is not None:
                if pCurMP.mnId == L:
                    self.step0_same += 1
                self.Replace(pCurMP.mnId, L, (-1, self.cur_kf, i))
            elif self.ref.point(L) in pCur.mvpMapPoints:
                self.n_matched_skipped += 1          # the deliberate difference: see the header
            else:
                self.ref.SetMapPointMatches(self.cur_kf, [i], [L])    # AddMapPoint + AddObservation
                self.ops.append((-1, 1, L, -1, self.cur_kf, i))
                self.ComputeDistinctiveDescriptors(L)
        self._check_final_rows()

    def _check_final_rows(self):
        """A survivor's row when the step ends, recomputed from the observers it has then, is the one its last
        Replace / add left: recomputing once per step is what recomputing inside every Replace gives."""
        if self.plan_first:                          # the wrong adapter promises nothing
            return
        for p, row in self.recomputed.items():
            assert np.array_equal(self.t["desc"][p], row), p
            if self.isBad(p):
                continue
            rows = np.stack([self.kf_desc[kf.mnId][idx] for kf, idx in self._observations(p)])
            assert np.array_equal(rows[restate_best(rows)], row), p

    # ---- ORBmatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) and the Replaces of SearchAndFuse
    def Fuse(self, c, kid, F, S8):
        pKF = self.ref.kfs[kid]
        vpPoints = self.loop_pts
        n = len(vpPoints)
        desc = self.start_desc if self.plan_first else self.t["desc"]
        bad = self.start_bad if self.plan_first else self.t["bad"]
        spAlreadyFound = set(m.mnId for m in pKF.mvpMapPoints if m is not None and not self.isBad(m.mnId))
        skip0 = np.array([p < 0 or bool(bad[p]) or p in spAlreadyFound for p in vpPoints], np.uint8)
        best = np.full(n, -1, np.int32)
        if n and not skip0.all():
            ids = np.asarray(vpPoints, np.int64)
            row = np.where(ids < 0, 0, ids)
            pts = MapPoints(self.t["pos"][row], desc[row], np.ones(n, np.int32))
            geo = MapPointGeo(self.t["max_dist"][row], self.t["min_dist"][row], self.t["normal"][row])
            _, best = oracle_lib.oracle_fuse_sim3(F, cvScw_of(S8), pts, geo, skip0, self.lsf, self.th)
        vpReplacePoint = [None] * n
        nFused, taken = 0, set()
        loop = set(p for p in vpPoints if p >= 0)
        for i, p in enumerate(vpPoints):
            if p < 0:
                continue
            now = self.isBad(p) or p in spAlreadyFound
            if not self.plan_first:
                assert now == bool(skip0[i]), (c, i, p)      # isBad of an examined point does not move inside a pass
            if skip0[i]:
                continue
            bestIdx = int(best[i])
            if bestIdx < 0:
                continue
            self.same_keypoint += bestIdx in taken
            taken.add(bestIdx)
            pMPinKF = pKF.mvpMapPoints[bestIdx]
            if pMPinKF is not None:
                q = pMPinKF.mnId
                if not self.isBad(q):
                    vpReplacePoint[i] = (q, bestIdx)
                else:
                    self.ops.append((c, 3, p, q, kid, bestIdx))
            else:
                self.ref.SetMapPointMatches(kid, [bestIdx], [p])    # AddObservation + AddMapPoint
                self.ops.append((c, 1, p, -1, kid, bestIdx))
            nFused += 1
        # no point with a non-NULL vpReplacePoint is itself a replace target of this pass
        targets = set(r[0] for r in vpReplacePoint if r is not None)
        assert self.plan_first or not any(r is not None and vpPoints[i] in targets
                                          for i, r in enumerate(vpReplacePoint)), c
        self.recomputed = {}
        self.replaced = set()
        for i, r in enumerate(vpReplacePoint):
            if r is not None:
                self.loop_by_loop += r[0] in loop
                self.Replace(r[0], vpPoints[i], (c, kid, r[1]))
        self._check_final_rows()
        return nFused

    # ---- CorrectLoop's fusion part
    def run(self):
        self.replaced = set()
        if self.matched is not None:
            self.step0()
        self.n_step0_ops = len(self.ops)
        for c in sorted(range(len(self.kf)), key=lambda j: self.kf[j]):      # id order for the address order
            self.nfused[c] = self.Fuse(c, self.kf[c], self.frames[c], self.Scw[c])
        return self

    def result(self):
        return dict(nfused=np.array(self.nfused, np.int32), ops=np.array(self.ops, np.int32).reshape(-1, 6),
                    updated=np.array(sorted(self.updated), np.int32), n_matched_skipped=self.n_matched_skipped)
