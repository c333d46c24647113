"""A literal restatement of LocalMapping::KeyFrameCulling and MapPointCulling (src/LocalMapping.cc) with
the parts of KeyFrame::SetBadFlag (src/KeyFrame.cc) and MapPoint::EraseObservation / SetBadFlag /
Observations (src/MapPoint.cc) they run through, on top of tests/map_ref.py.

A keyframe carries mvKeysUn[i].octave, whether mvuRight[i] >= 0 (stereo) and whether mvDepth[i] is beyond
mThDepth or negative (far), per slot.  nObs is formed from mObservations where it is read: 2 per stereo
observation, 1 per monocular one, which is what the reference's counter holds.  Plain Python over the
objects of map_ref; nothing is shared with the library."""
import numpy as np

from map_ref import RefMap


class CullRefMap(RefMap):
    # ---- mutations
    def AddKeyFrame(self, kid, mp, observed=None):
        super().AddKeyFrame(kid, mp, observed)
        kf = self.kfs[kid]
        n = len(kf.mvpMapPoints)
        kf.octave, kf.stereo, kf.far = [0] * n, [False] * n, [False] * n   # keys never set

    def SetKeyFrameKeys(self, kid, octave, uRight=None, depth=None, thDepth=0.0):
        kf = self.kfs[kid]
        n = len(kf.mvpMapPoints)
        assert len(octave) == n
        kf.octave = [int(o) for o in octave]
        kf.stereo = [False] * n if uRight is None else [bool(np.float32(u) >= 0) for u in uRight]
        th = np.float32(thDepth)
        kf.far = [False] * n if depth is None else [bool(np.float32(d) > th or np.float32(d) < 0) for d in depth]

    # ---- MapPoint
    @staticmethod
    def Observations(pMP):
        return sum(2 if pKF.stereo[idx] else 1 for pKF, idx in pMP.mObservations.items())

    def _MapPoint_SetBadFlag(self, pMP):
        obs = dict(pMP.mObservations)
        pMP.mObservations.clear()
        pMP.mbBad = True
        for pKF, idx in obs.items():
            pKF.mvpMapPoints[idx] = None                      # KeyFrame::EraseMapPointMatch

    def _MapPoint_EraseObservation(self, pMP, pKF, went_bad):
        bBad = False
        if pKF in pMP.mObservations:
            del pMP.mObservations[pKF]                        # nObs -= 2 or 1
            if self.Observations(pMP) <= 2:
                bBad = True
        if bBad:
            self._MapPoint_SetBadFlag(pMP)
            went_bad.append(pMP.mnId)

    def _KeyFrame_SetBadFlag(self, pKF, went_bad):
        for i in range(len(pKF.mvpMapPoints)):
            if pKF.mvpMapPoints[i] is not None:
                self._MapPoint_EraseObservation(pKF.mvpMapPoints[i], pKF, went_bad)
        pKF.mbBad = True

    # ---- LocalMapping::KeyFrameCulling
    def KeyFrameCulling(self, cand, not_erase=None, monocular=False):
        """-> dict(nMPs, nRedundant, verdict, bad_mp); the map is changed as the reference changes it."""
        out_mps, out_red, verdict, went_bad = [], [], [], []
        for c, kid in enumerate(cand):
            kid = int(kid)
            pKF = self.live(kid)
            if kid == 0 or pKF is None:
                out_mps.append(0)
                out_red.append(0)
                verdict.append(3)
                continue
            thObs = 3
            nRedundantObservations = 0
            nMPs = 0
            for i in range(len(pKF.mvpMapPoints)):
                pMP = pKF.mvpMapPoints[i]
                if pMP is not None:
                    if not pMP.isBad():
                        if not monocular:
                            if pKF.far[i]:
                                continue
                        nMPs += 1
                        if self.Observations(pMP) > thObs:
                            scaleLevel = pKF.octave[i]
                            nObs = 0
                            for pKFi, idx in pMP.mObservations.items():
                                if pKFi is pKF:
                                    continue
                                scaleLeveli = pKFi.octave[idx]
                                if scaleLeveli <= scaleLevel + 1:
                                    nObs += 1
                                    if nObs >= thObs:
                                        break
                            if nObs >= thObs:
                                nRedundantObservations += 1
            out_mps.append(nMPs)
            out_red.append(nRedundantObservations)
            if nRedundantObservations > 0.9 * nMPs:
                if not_erase is not None and not_erase[c]:
                    verdict.append(2)                         # mbToBeErased
                else:
                    self._KeyFrame_SetBadFlag(pKF, went_bad)
                    verdict.append(1)
            else:
                verdict.append(0)
        return dict(nMPs=out_mps, nRedundant=out_red, verdict=verdict, bad_mp=went_bad)

    # ---- LocalMapping::MapPointCulling
    def MapPointCulling(self, mp, first_kf, found, visible, cur_kf, monocular=False):
        """-> (verdict, observations as read before the call); SetBadFlag is run where the reference runs it."""
        cnThObs = 2 if monocular else 3
        verdict, observations = [], []
        todo = []
        for p, first, nf, nv in zip(mp, first_kf, found, visible):
            pMP = self.pts.get(int(p))
            nobs = self.Observations(pMP) if pMP is not None else 0
            observations.append(nobs)
            ratio = np.float32(nf) / np.float32(nv)
            age = int(cur_kf) - int(first)
            if pMP is not None and pMP.isBad():
                verdict.append(1)
            elif ratio < np.float32(0.25):
                verdict.append(2)
                todo.append(int(p))
            elif age >= 2 and nobs <= cnThObs:
                verdict.append(3)
                todo.append(int(p))
            elif age >= 3:
                verdict.append(4)
            else:
                verdict.append(0)
        for p in todo:
            self._MapPoint_SetBadFlag(self.point(p))
        return verdict, observations
