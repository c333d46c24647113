"""A literal, stateful restatement of the part of ORB-SLAM2 that relates keyframes and map points,
and of the two functions that count over it: Tracking::UpdateLocalMap (UpdateLocalKeyFrames +
UpdateLocalPoints, Tracking.cc:1195-1339) and KeyFrame::UpdateConnections (KeyFrame.cc).

Objects, loops and breaks are transcribed as the reference has them: mObservations and
mvpMapPoints are kept separately, the marks are mnTrackReferenceForFrame, the ordered list is the
ascending sort of (weight, keyframe) pushed to the front.  Where the reference iterates a
pointer-keyed std::map / std::set, ascending id stands in for the address order.  The module
shares nothing with the library: it is plain Python over dicts and lists."""


class MapPoint:
    def __init__(self, mnId):
        self.mnId = mnId
        self.mObservations = {}   # KeyFrame -> idx
        self.mbBad = False
        self.mnTrackReferenceForFrame = -1

    def isBad(self):
        return self.mbBad

    def AddObservation(self, pKF, idx):
        if pKF in self.mObservations:
            return
        self.mObservations[pKF] = idx

    def EraseObservation(self, pKF):
        self.mObservations.pop(pKF, None)

    def IsInKeyFrame(self, pKF):
        return pKF in self.mObservations


class KeyFrame:
    def __init__(self, mnId, n):
        self.mnId = mnId
        self.mvpMapPoints = [None] * n
        self.mbBad = False
        self.best10 = []          # ids, as forwarded: the first <= 10 of mvpOrderedConnectedKeyFrames
        self.parent = -1          # id
        self.children = []        # ids
        self.mnTrackReferenceForFrame = -1

    def isBad(self):
        return self.mbBad


class RefMap:
    def __init__(self):
        self.kfs = {}      # id -> KeyFrame (bad ones stay, flagged)
        self.pts = {}      # id -> MapPoint
        self.frame_id = 0

    def point(self, p):
        if p not in self.pts:
            self.pts[p] = MapPoint(p)
        return self.pts[p]

    def live(self, kid):
        kf = self.kfs.get(kid)
        return kf if kf is not None and not kf.isBad() else None

    # ---- mutations, named after the library's entries
    def AddKeyFrame(self, kid, mp, observed=None):
        assert self.live(kid) is None
        kf = KeyFrame(kid, len(mp))
        self.kfs[kid] = kf
        for i, p in enumerate(mp):
            if p < 0:
                continue
            pMP = self.point(int(p))
            kf.mvpMapPoints[i] = pMP                      # Tracking::CreateNewKeyFrame
            if observed is None or observed[i]:
                pMP.AddObservation(kf, i)                 # LocalMapping::ProcessNewKeyFrame

    def SetMapPointMatches(self, kid, slots, mp, observed=None):
        kf = self.kfs[kid]
        for k, (s, p) in enumerate(zip(slots, mp)):       # the sources of a move empty first
            if p < 0:
                self._empty(kf, int(s))
        for k, (s, p) in enumerate(zip(slots, mp)):
            s, p = int(s), int(p)
            if p < 0:
                continue
            self._empty(kf, s)
            pMP = self.point(p)
            kf.mvpMapPoints[s] = pMP                      # KeyFrame::AddMapPoint / ReplaceMapPointMatch
            if observed is None or observed[k]:
                pMP.AddObservation(kf, s)

    @staticmethod
    def _empty(kf, s):
        old = kf.mvpMapPoints[s]
        if old is not None and old.mObservations.get(kf) == s:
            old.EraseObservation(kf)
        kf.mvpMapPoints[s] = None                         # KeyFrame::EraseMapPointMatch

    def EraseMapPoint(self, p):
        """MapPoint::SetBadFlag"""
        pMP = self.point(p)
        obs = dict(pMP.mObservations)
        pMP.mObservations.clear()
        pMP.mbBad = True
        for pKF, idx in obs.items():
            pKF.mvpMapPoints[idx] = None

    def ReplaceMapPoint(self, p, by):
        """MapPoint::Replace; 'already in that keyframe' is read off the keyframe's row, as the
        library's specification states it."""
        if p == by:
            return
        pMP, pBy = self.point(p), self.point(by)
        obs = dict(pMP.mObservations)
        pMP.mObservations.clear()
        pMP.mbBad = True
        for pKF, idx in sorted(obs.items(), key=lambda kv: kv[0].mnId):
            if pBy not in pKF.mvpMapPoints:
                pKF.mvpMapPoints[idx] = pBy
                pBy.AddObservation(pKF, idx)
            else:
                pKF.mvpMapPoints[idx] = None

    def EraseKeyFrame(self, kid):
        """KeyFrame::SetBadFlag (the observation part)"""
        kf = self.kfs[kid]
        for pMP in kf.mvpMapPoints:
            if pMP is not None:
                pMP.EraseObservation(kf)
        kf.mbBad = True

    def SetNeighbours(self, kid, best10, parent=-1, children=()):
        kf = self.kfs[kid]
        kf.best10 = [int(x) for x in best10][:10]
        kf.parent = int(parent)
        kf.children = sorted(int(c) for c in children)    # std::set<KeyFrame*>: id for address order

    # ---- KeyFrame::UpdateConnections
    def UpdateConnections(self, kid):
        this = self.kfs[kid]
        KFcounter = {}
        for pMP in this.mvpMapPoints:
            if pMP is None:
                continue
            if pMP.isBad():
                continue
            for pKF in pMP.mObservations:
                if pKF.mnId == this.mnId:
                    continue
                KFcounter[pKF] = KFcounter.get(pKF, 0) + 1
        counter = sorted(KFcounter.items(), key=lambda kv: kv[0].mnId)
        counter_id = [k.mnId for k, _ in counter]
        counter_n = [c for _, c in counter]
        if not KFcounter:
            return counter_id, counter_n, [], []
        nmax, pKFmax, th = 0, None, 15
        vPairs = []
        for pKF, c in counter:
            if c > nmax:
                nmax = c
                pKFmax = pKF
            if c >= th:
                vPairs.append((c, pKF.mnId))
        if not vPairs:
            vPairs.append((nmax, pKFmax.mnId))
        vPairs.sort()
        lKFs, lWs = [], []
        for w, k in vPairs:
            lKFs.insert(0, k)     # push_front
            lWs.insert(0, w)
        return counter_id, counter_n, lKFs, lWs

    # ---- Tracking::UpdateLocalMap
    def UpdateLocalMap(self, cur_mp):
        """cur_mp: list of global ids (-1 = NULL), modified in place as mCurrentFrame.mvpMapPoints is.
        -> None for an empty vote, else dict(local_kf, ref_kf, local_mp, cur_row)."""
        self.frame_id += 1
        fid = self.frame_id
        mvp = [self.point(int(p)) if p >= 0 else None for p in cur_mp]
        # UpdateLocalKeyFrames
        keyframeCounter = {}
        for i in range(len(mvp)):
            if mvp[i] is not None:
                pMP = mvp[i]
                if not pMP.isBad():
                    for pKF in pMP.mObservations:
                        keyframeCounter[pKF] = keyframeCounter.get(pKF, 0) + 1
                else:
                    mvp[i] = None
                    cur_mp[i] = -1
        if not keyframeCounter:
            return None
        mx, pKFmax = 0, None
        local = []
        for pKF in sorted(keyframeCounter, key=lambda k: k.mnId):
            if pKF.isBad():
                continue
            if keyframeCounter[pKF] > mx:
                mx = keyframeCounter[pKF]
                pKFmax = pKF
            local.append(pKF)
            pKF.mnTrackReferenceForFrame = fid
        end = len(local)
        for t in range(end):
            if len(local) > 80:
                break
            pKF = local[t]
            for nid in pKF.best10:
                pNeighKF = self.live(nid)
                if pNeighKF is not None:
                    if pNeighKF.mnTrackReferenceForFrame != fid:
                        local.append(pNeighKF)
                        pNeighKF.mnTrackReferenceForFrame = fid
                        break
            for cid in pKF.children:
                pChildKF = self.live(cid)
                if pChildKF is not None:
                    if pChildKF.mnTrackReferenceForFrame != fid:
                        local.append(pChildKF)
                        pChildKF.mnTrackReferenceForFrame = fid
                        break
            pParent = self.live(pKF.parent)
            if pParent is not None:
                if pParent.mnTrackReferenceForFrame != fid:
                    local.append(pParent)
                    pParent.mnTrackReferenceForFrame = fid
                    break       # leaves the loop over the keyframes
        # UpdateLocalPoints
        local_mp = []
        for pKF in local:
            for pMP in pKF.mvpMapPoints:
                if pMP is None:
                    continue
                if pMP.mnTrackReferenceForFrame == fid:
                    continue
                if not pMP.isBad():
                    local_mp.append(pMP)
                    pMP.mnTrackReferenceForFrame = fid
        rowof = {pMP: j for j, pMP in enumerate(local_mp)}
        cur_row = [rowof.get(m, -1) if m is not None else -1 for m in mvp]
        return dict(local_kf=[k.mnId for k in local], ref_kf=pKFmax.mnId if pKFmax is not None else -1,
                    local_mp=[m.mnId for m in local_mp], cur_row=cur_row)

    def bad_flags(self, n):
        import numpy as np
        b = np.zeros(n, np.uint8)
        for p, m in self.pts.items():
            if m.isBad() and p < n:
                b[p] = 1
        return b
