"""A literal, stateful restatement of the reference's KeyFrameDatabase (src/KeyFrameDatabase.cc) in
Python: the inverted file as a list of lists of keyframes, the marking fields on the keyframes,
float arithmetic through numpy.float32 and L1Scoring::score (ScoringObject.cpp:21-66) in float64
in the reference's merge order.  It walks the inverted file exactly as the reference does and does
NOT use the closed-form order of lKFsSharingWords: the library's closed form is checked against it.

Two deliberate deviations, the ones include/orbslam_gpu.h and DESIGN.md §3.10 name:
  - DetectRelocalizationCandidates counts a neighbour only if it was scored in this query (the
    reference reads mRelocScore of any neighbour marked by this frame, scored or not);
  - a query is identified by a token of its own, so the marking fields' initial value never aliases
    a query id of 0."""
from bisect import bisect_left

import numpy as np

f32 = np.float32


def l1_score(v1, v2):
    """double L1Scoring::score(const BowVector& v1, const BowVector& v2); v = (words, values)."""
    w1, x1 = v1
    w2, x2 = v2
    n1, n2 = len(w1), len(w2)
    i1 = i2 = 0
    score = 0.0
    while i1 < n1 and i2 < n2:
        if w1[i1] == w2[i2]:
            vi, wi = float(x1[i1]), float(x2[i2])
            score += abs(vi - wi) - abs(vi) - abs(wi)
            i1 += 1
            i2 += 1
        elif w1[i1] < w2[i2]:
            i1 = bisect_left(w1, w2[i2], i1)      # v1.lower_bound(v2_it->first)
        else:
            i2 = bisect_left(w2, w1[i1], i2)
    return -score / 2.0


class RefKeyFrame:
    def __init__(self, mnId):
        self.mnId = mnId
        self.mBowVec = ([], [])                   # ascending words, values
        self.mvpOrderedConnectedKeyFrames = []
        self.mnLoopQuery = None
        self.mnLoopWords = 0
        self.mLoopScore = f32(0)
        self.mnRelocQuery = None
        self.mnRelocWords = 0
        self.mRelocScore = f32(0)

    def GetBestCovisibilityKeyFrames(self, N):
        return self.mvpOrderedConnectedKeyFrames[:N]


class RefStages:
    """What the library reports as stage outputs, plus the order of lKFsSharingWords."""

    def __init__(self):
        self.sharing_ids = []
        self.n_sharing = 0
        self.maxCommonWords = 0
        self.minCommonWords = 0
        self.scored_id, self.scored_words, self.scored_score, self.scored_acc = [], [], [], []
        self.n_scored = 0
        self.bestAccScore = f32(0)
        self.n_score_and_match = 0
        self.acc_best = []                        # (accScore, best id, entry id) per lScoreAndMatch entry
        self.cand = []


class RefKeyFrameDatabase:
    def __init__(self, n_words):
        self.mvInvertedFile = [[] for _ in range(n_words)]
        self.keyframes = {}                       # the map's keyframes by id, in the database or not

    def kf(self, mnId):
        if mnId not in self.keyframes:
            self.keyframes[mnId] = RefKeyFrame(mnId)
        return self.keyframes[mnId]

    def set_covisibles(self, mnId, ids):
        self.kf(mnId).mvpOrderedConnectedKeyFrames = [self.kf(i) for i in ids]

    def add(self, pKF):                            # 39-45
        for w in pKF.mBowVec[0]:
            self.mvInvertedFile[w].append(pKF)

    def erase(self, pKF):                          # 47-67
        for w in pKF.mBowVec[0]:
            lKFs = self.mvInvertedFile[w]
            for i, k in enumerate(lKFs):
                if k is pKF:
                    del lKFs[i]
                    break

    def clear(self):                               # 69-73
        self.mvInvertedFile = [[] for _ in range(len(self.mvInvertedFile))]

    def DetectLoopCandidates(self, bow, connected_ids, minScore):   # 76-197
        minScore = f32(minScore)
        query = object()
        st = RefStages()
        st.bestAccScore = minScore
        spConnectedKeyFrames = set(connected_ids)
        lKFsSharingWords = []
        for w in bow[0]:
            for pKFi in self.mvInvertedFile[w]:
                if pKFi.mnLoopQuery is not query:
                    pKFi.mnLoopWords = 0
                    if pKFi.mnId not in spConnectedKeyFrames:
                        pKFi.mnLoopQuery = query
                        lKFsSharingWords.append(pKFi)
                pKFi.mnLoopWords += 1
        st.sharing_ids = [k.mnId for k in lKFsSharingWords]
        st.n_sharing = len(lKFsSharingWords)
        if not lKFsSharingWords:
            return st
        maxCommonWords = 0
        for k in lKFsSharingWords:
            if k.mnLoopWords > maxCommonWords:
                maxCommonWords = k.mnLoopWords
        minCommonWords = int(f32(maxCommonWords) * f32(0.8))
        st.maxCommonWords, st.minCommonWords = maxCommonWords, minCommonWords
        lScoreAndMatch = []
        scored = []
        for pKFi in lKFsSharingWords:
            if pKFi.mnLoopWords > minCommonWords:
                si = f32(l1_score(bow, pKFi.mBowVec))
                pKFi.mLoopScore = si
                scored.append(pKFi)
                if si >= minScore:
                    lScoreAndMatch.append((si, pKFi))
        self._stage_scored(st, scored, "mnLoopWords", "mLoopScore")
        if not lScoreAndMatch:
            return st
        lAccScoreAndMatch = []
        bestAccScore = minScore
        for si, pKFi in lScoreAndMatch:
            bestScore = si
            accScore = si
            pBestKF = pKFi
            for pKF2 in pKFi.GetBestCovisibilityKeyFrames(10):
                if pKF2.mnLoopQuery is query and pKF2.mnLoopWords > minCommonWords:
                    accScore = f32(accScore + pKF2.mLoopScore)
                    if pKF2.mLoopScore > bestScore:
                        pBestKF = pKF2
                        bestScore = pKF2.mLoopScore
            lAccScoreAndMatch.append((accScore, pBestKF))
            st.acc_best.append((accScore, pBestKF.mnId, pKFi.mnId))
            if accScore > bestAccScore:
                bestAccScore = accScore
        return self._retain(st, scored, lScoreAndMatch, lAccScoreAndMatch, bestAccScore)

    def DetectRelocalizationCandidates(self, bow):   # 199-309
        query = object()
        st = RefStages()
        lKFsSharingWords = []
        for w in bow[0]:
            for pKFi in self.mvInvertedFile[w]:
                if pKFi.mnRelocQuery is not query:
                    pKFi.mnRelocWords = 0
                    pKFi.mnRelocQuery = query
                    lKFsSharingWords.append(pKFi)
                pKFi.mnRelocWords += 1
        st.sharing_ids = [k.mnId for k in lKFsSharingWords]
        st.n_sharing = len(lKFsSharingWords)
        if not lKFsSharingWords:
            return st
        maxCommonWords = 0
        for k in lKFsSharingWords:
            if k.mnRelocWords > maxCommonWords:
                maxCommonWords = k.mnRelocWords
        minCommonWords = int(f32(maxCommonWords) * f32(0.8))
        st.maxCommonWords, st.minCommonWords = maxCommonWords, minCommonWords
        lScoreAndMatch = []
        scored = []
        for pKFi in lKFsSharingWords:
            if pKFi.mnRelocWords > minCommonWords:
                si = f32(l1_score(bow, pKFi.mBowVec))
                pKFi.mRelocScore = si
                scored.append(pKFi)
                lScoreAndMatch.append((si, pKFi))
        self._stage_scored(st, scored, "mnRelocWords", "mRelocScore")
        if not lScoreAndMatch:
            return st
        lAccScoreAndMatch = []
        bestAccScore = f32(0)
        for si, pKFi in lScoreAndMatch:
            bestScore = si
            accScore = bestScore
            pBestKF = pKFi
            for pKF2 in pKFi.GetBestCovisibilityKeyFrames(10):
                if pKF2.mnRelocQuery is not query:
                    continue
                if not pKF2.mnRelocWords > minCommonWords:   # deviation 1: scored in this query only
                    continue
                accScore = f32(accScore + pKF2.mRelocScore)
                if pKF2.mRelocScore > bestScore:
                    pBestKF = pKF2
                    bestScore = pKF2.mRelocScore
            lAccScoreAndMatch.append((accScore, pBestKF))
            st.acc_best.append((accScore, pBestKF.mnId, pKFi.mnId))
            if accScore > bestAccScore:
                bestAccScore = accScore
        return self._retain(st, scored, lScoreAndMatch, lAccScoreAndMatch, bestAccScore)

    @staticmethod
    def _stage_scored(st, scored, words, score):
        st.scored_id = [k.mnId for k in scored]
        st.scored_words = [getattr(k, words) for k in scored]
        st.scored_score = [getattr(k, score) for k in scored]
        st.scored_acc = [f32(np.nan)] * len(scored)
        st.n_scored = len(scored)

    @staticmethod
    def _retain(st, scored, lScoreAndMatch, lAccScoreAndMatch, bestAccScore):   # 180-194, 292-306
        st.bestAccScore = bestAccScore
        st.n_score_and_match = len(lScoreAndMatch)
        pos = {id(k): i for i, k in enumerate(scored)}
        for (acc, _), (_, pKFi) in zip(lAccScoreAndMatch, lScoreAndMatch):
            st.scored_acc[pos[id(pKFi)]] = acc
        minScoreToRetain = f32(f32(0.75) * bestAccScore)
        spAlreadyAddedKF = set()
        for acc, pKFi in lAccScoreAndMatch:
            if acc > minScoreToRetain:
                if pKFi.mnId not in spAlreadyAddedKF:
                    st.cand.append(pKFi.mnId)
                    spAlreadyAddedKF.add(pKFi.mnId)
        return st


def run_steps(steps, n_words):
    """Apply a case's steps (kfdb_cases) to a fresh restatement; the stages of every query step."""
    db = RefKeyFrameDatabase(n_words)
    in_db = set()
    out = []
    for s in steps:
        op = s[0]
        if op == "add":
            k = db.kf(s[1])
            k.mBowVec = (s[2][0].tolist(), s[2][1].tolist())
            db.add(k)
            in_db.add(s[1])
        elif op == "add_batch":
            for i, b in zip(s[1], s[2]):
                k = db.kf(i)
                k.mBowVec = (b[0].tolist(), b[1].tolist())
                db.add(k)
                in_db.add(i)
        elif op == "erase":
            if s[1] in in_db:                     # the library: erasing an absent id does nothing
                db.erase(db.keyframes[s[1]])
                in_db.discard(s[1])
        elif op == "clear":
            db.clear()
            in_db.clear()
        elif op == "cov":
            db.set_covisibles(s[1], s[2])
        elif op == "loop":
            out.append(db.DetectLoopCandidates((s[1][0].tolist(), s[1][1].tolist()), s[2], s[3]))
        elif op == "reloc":
            out.append(db.DetectRelocalizationCandidates((s[1][0].tolist(), s[1][1].tolist())))
        elif op == "reloc_batch":
            out.append([db.DetectRelocalizationCandidates((b[0].tolist(), b[1].tolist())) for b in s[1]])
        else:
            raise ValueError(op)
    return out
