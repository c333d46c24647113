"""A literal restatement of LocalMapping::SearchInNeighbors (src/LocalMapping.cc:454-553) from the parts the
suite already has: the relation and MapPoint::Replace of map_ref.RefMap, nObs as culling_ref counts it, the
per-pass selection of ORBmatcher::Fuse (src/ORBmatcher.cc:825-949) by the CPU oracle, and
ComputeDistinctiveDescriptors / UpdateNormalAndDepth as localmap_ref restates them.

Everything runs where the reference runs it: the mutations inside the loop over the points, the skip tests
at each point's turn, ComputeDistinctiveDescriptors inside Replace.  The oracle is asked once per pass with
the skip flags of the pass's start; that the two agree at every point's turn is asserted, not assumed.

stale=True freezes the descriptors the passes match with at their starting values: the plan-all-targets-first
adapter this entry exists to replace.  Nothing here is shared with the library."""
import numpy as np

import oracle_lib
from c_orb_slam_amd.orb import MapPointGeo, MapPoints
from localmap_ref import ref64_normal_depth, restate_best, restate_normal_depth


class SearchInNeighborsRef:
    def __init__(self, ref, cur_kf, cur, target_ids, targets, kf_desc, Ow, scale_factors, table, logScaleFactor,
                 th=3.0, stale=False):
        """ref: a culling_ref.CullRefMap (changed as the reference changes the map); table: dict of arrays,
        copied here.  The results are the attributes t (the table), ops, nfused, updated, n_ref_missing."""
        self.ref, self.cur_kf, self.cur = ref, int(cur_kf), cur
        self.target_ids, self.targets = [int(t) for t in target_ids], list(targets)
        self.kf_desc, self.Ow = kf_desc, np.asarray(Ow, np.float32).reshape(-1, 3)
        self.sf = np.asarray(scale_factors, np.float32)
        self.t = {k: np.array(v, copy=True) for k, v in table.items()}
        self.start_desc = self.t["desc"].copy()
        self.lsf, self.th, self.stale = np.float32(logScaleFactor), float(th), stale
        self.ops, self.nfused, self.updated, self.n_ref_missing = [], [], set(), 0
        self.final_rows = {}     # point -> the inputs of its UpdateNormalAndDepth (for a float64 check)
        self.same_keypoint = 0   # points fused onto a keypoint another point of the same pass took
        self.replaced_examined = self.replaced_held = 0   # the two directions of Replace

    # ---- MapPoint
    def isBad(self, p):
        return bool(self.t["bad"][p])

    def Observations(self, p):
        return self.ref.Observations(self.ref.point(p))

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
        self.t["desc"][p] = rows[restate_best(rows)]
        self.updated.add(p)

    def UpdateNormalAndDepth(self, p):
        if self.isBad(p):
            return
        obs = self._observations(p)
        if not obs:
            return
        r = int(self.t["ref_kf"][p])
        at = [idx for kf, idx in obs if kf.mnId == r]
        if r < 0 or not at or self.ref.kfs[r].octave[at[0]] >= len(self.sf):
            self.n_ref_missing += 1
            return
        args = (self.t["pos"][p], self.Ow[[kf.mnId for kf, _ in obs]], self.Ow[r],
                self.sf[self.ref.kfs[r].octave[at[0]]], self.sf[-1])
        n, mx, mn = restate_normal_depth(*args)
        self.t["normal"][p], self.t["max_dist"][p], self.t["min_dist"][p] = n, mx, mn
        self.final_rows[p] = args
        self.updated.add(p)

    def Replace(self, a, b, where):
        """a->Replace(b) (MapPoint.cc): Map_ReplaceMapPoint's relation change, the flag, the descriptor"""
        self.ref.ReplaceMapPoint(a, b)
        self.t["bad"][a] = 1
        self.updated.add(a)
        self.ops.append((where[0], 2, a, b, where[1], where[2]))
        self.survivors.add(b)
        self.ComputeDistinctiveDescriptors(b)

    # ---- ORBmatcher::Fuse(pKF, vpMapPoints, th)
    def Fuse(self, kid, F, vpMapPoints, pass_idx):
        pKF = self.ref.kfs[kid]
        n = len(vpMapPoints)
        ids = np.asarray(vpMapPoints, np.int64)
        skip0 = np.array([p < 0 or self.isBad(p) or self.ref.point(p).IsInKeyFrame(pKF) for p in vpMapPoints], np.uint8)
        best = np.full(n, -1, np.int32)
        if n and not skip0.all():
            row = np.where(ids < 0, 0, ids)
            desc = self.start_desc if self.stale else self.t["desc"]
            pts = MapPoints(self.t["pos"][row], desc[row], np.ones(n, np.int32))
            geo = MapPointGeo(self.t["max_dist"][row], self.t["min_dist"][row], self.t["normal"][row])
            _, best = oracle_lib.oracle_fuse(F, pts, geo, skip0, self.lsf, self.th)
        nFused, taken = 0, set()
        self.survivors = set()       # of this pass
        for i, p in enumerate(vpMapPoints):
            if p < 0:
                continue
            now = self.isBad(p) or self.ref.point(p).IsInKeyFrame(pKF)
            assert now == bool(skip0[i]), (pass_idx, i, p)      # the skip test does not move inside a pass
            if now:
                continue
            assert p not in self.survivors, (pass_idx, i, p)    # so its descriptor is the one the pass started with
            bestIdx = int(best[i])
            if bestIdx < 0:
                continue
            self.same_keypoint += bestIdx in taken
            taken.add(bestIdx)
            pMPinKF = pKF.mvpMapPoints[bestIdx]
            where = (pass_idx, kid, bestIdx)
            if pMPinKF is not None:
                q = pMPinKF.mnId
                if not self.isBad(q):
                    if self.Observations(q) > self.Observations(p):
                        self.Replace(p, q, where)
                        self.replaced_examined += 1
                    else:
                        self.Replace(q, p, where)
                        self.replaced_held += 1
                else:
                    self.ops.append((pass_idx, 3, p, q, kid, bestIdx))
            else:
                self.ref.SetMapPointMatches(kid, [bestIdx], [p])    # AddObservation + AddMapPoint
                self.ops.append((pass_idx, 1, p, -1, kid, bestIdx))
            nFused += 1
        return nFused

    # ---- LocalMapping::SearchInNeighbors
    def run(self):
        ref = self.ref
        pCur = ref.kfs[self.cur_kf]
        vpMapPointMatches = [-1 if m is None else m.mnId for m in pCur.mvpMapPoints]
        for t, (kid, F) in enumerate(zip(self.target_ids, self.targets)):
            self.nfused.append(self.Fuse(kid, F, vpMapPointMatches, t))
        vpFuseCandidates, mnFuseCandidateForKF = [], set()
        for kid in self.target_ids:
            for pMP in ref.kfs[kid].mvpMapPoints:
                if pMP is None:
                    continue
                if self.isBad(pMP.mnId) or pMP.mnId in mnFuseCandidateForKF:
                    continue
                mnFuseCandidateForKF.add(pMP.mnId)
                vpFuseCandidates.append(pMP.mnId)
        self.n_candidates = len(vpFuseCandidates)
        self.nfused.append(self.Fuse(self.cur_kf, self.cur, vpFuseCandidates, len(self.target_ids)))
        for pMP in list(pCur.mvpMapPoints):
            if pMP is not None:
                if not self.isBad(pMP.mnId):
                    self.ComputeDistinctiveDescriptors(pMP.mnId)
                    self.UpdateNormalAndDepth(pMP.mnId)
        return self

    def result(self):
        return dict(nfused=np.array(self.nfused, np.int32), ops=np.array(self.ops, np.int32).reshape(-1, 6),
                    updated=np.array(sorted(self.updated), np.int32), n_ref_missing=self.n_ref_missing)

    def float64_deviation(self, normal, max_dist, min_dist):
        """The worst deviation of the given rows from the float64 formulas, each in units of the bound
        tests/test_localmap_cpu.py sets for the restatement: (k + 3) * 2^-24 absolute for a normal over k
        observations, 4 * 2^-24 relative for max_dist, 6 * 2^-24 relative for min_dist."""
        worst = 0.0
        for p, args in self.final_rows.items():
            n64, mx64, mn64 = ref64_normal_depth(*args)
            k = len(args[1])
            worst = max(worst, float(np.abs(np.asarray(normal[p], np.float64) - n64).max()) / ((k + 3) * 2.0 ** -24),
                        abs(float(max_dist[p]) - mx64) / (4 * 2.0 ** -24 * mx64),
                        abs(float(min_dist[p]) - mn64) / (6 * 2.0 ** -24 * mn64))
        return worst
