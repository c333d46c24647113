"""Host-side mirror of the reference's KeyFrameDatabase (include/KeyFrameDatabase.h,
src/KeyFrameDatabase.cc): add / erase / clear and the two candidate searches.  The stored
BowVectors live in device memory; every call goes through the C ABI into the HIP library, which
scans them on the device and replays the list logic in the reference's order."""
import ctypes as C

import numpy as np

from ._lib import ORB_E_CAPACITY, OrbGpuError, check, lib, orb_kfdb_query, orb_kfdb_result, ptr
from .vocabulary import BowVector


class KfdbStages:
    """Stage outputs of one query: the scored subset (words > minCommonWords) in lKFsSharingWords
    order with mnLoopWords / mLoopScore, accScore (NaN where the entry did not reach
    lScoreAndMatch), and the thresholds."""

    def __init__(self, r, bufs):
        n = r.n_scored
        self.scored_id = bufs["id"][:n].copy()
        self.scored_words = bufs["words"][:n].copy()
        self.scored_score = bufs["score"][:n].copy()
        self.scored_acc = bufs["acc"][:n].copy()
        self.n_scored, self.n_sharing = r.n_scored, r.n_sharing
        self.maxCommonWords, self.minCommonWords = r.maxCommonWords, r.minCommonWords
        self.bestAccScore = np.float32(r.bestAccScore)


class KeyFrameDatabase:
    def __init__(self, voc):
        self._L = lib()
        self._voc = voc   # must outlive the database
        h = C.c_void_p()
        check(self._L.KeyFrameDatabase_create(voc._h, C.byref(h)), "KeyFrameDatabase_create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._L.KeyFrameDatabase_destroy(self._h)
            self._h = None

    __del__ = close

    def add(self, id, bow: BowVector):
        """void add(KeyFrame*) (39-45): id = pKF->mnId, bow = pKF->mBowVec."""
        check(self._L.KeyFrameDatabase_add(self._h, int(id), ptr(bow.words), ptr(bow.values), len(bow)),
              "KeyFrameDatabase_add")

    def add_batch(self, ids, bows):
        ids = np.ascontiguousarray(ids, np.int32)
        start = np.zeros(len(bows) + 1, np.int32)
        start[1:] = np.cumsum([len(b) for b in bows])
        w = np.concatenate([b.words for b in bows] + [np.zeros(1, np.uint32)])
        v = np.concatenate([b.values for b in bows] + [np.zeros(1)])
        check(self._L.KeyFrameDatabase_add_batch(self._h, len(bows), ptr(ids), ptr(start), ptr(w), ptr(v)),
              "KeyFrameDatabase_add_batch")

    def erase(self, id):
        check(self._L.KeyFrameDatabase_erase(self._h, int(id)), "KeyFrameDatabase_erase")

    def clear(self):
        check(self._L.KeyFrameDatabase_clear(self._h), "KeyFrameDatabase_clear")

    def size(self):
        """(live keyframes, BowVector entries they hold)"""
        n, e = C.c_int(), C.c_longlong()
        check(self._L.KeyFrameDatabase_size(self._h, C.byref(n), C.byref(e)), "KeyFrameDatabase_size")
        return n.value, e.value

    def set_covisibles(self, id, ids):
        """GetBestCovisibilityKeyFrames(10) of keyframe `id` (the first <= 10 ordered connections)."""
        a = np.ascontiguousarray(ids, np.int32)
        check(self._L.KeyFrameDatabase_set_covisibles(self._h, int(id), len(a), ptr(a) if len(a) else None),
              "KeyFrameDatabase_set_covisibles")

    def enable_timing(self, on=True):
        check(self._L.KeyFrameDatabase_enable_timing(self._h, int(on)), "KeyFrameDatabase_enable_timing")

    def last_timings(self):
        """ms of the last timed query: (share count and selection, scoring, whole call)."""
        ms = np.zeros(3, np.float32)
        check(self._L.KeyFrameDatabase_last_timings(self._h, ptr(ms)), "KeyFrameDatabase_last_timings")
        return ms

    # ---- queries
    @staticmethod
    def _query(bow, exclude=None, minScore=0.0):
        ex = np.ascontiguousarray(exclude if exclude is not None else [], np.int32)
        q = orb_kfdb_query(len(bow), ptr(bow.words) if len(bow) else None, ptr(bow.values) if len(bow) else None,
                           len(ex), ptr(ex) if len(ex) else None, float(minScore))
        return q, (bow, ex)

    @staticmethod
    def _result(cap, cap_scored):
        b = dict(cand=np.zeros(max(cap, 1), np.int32), id=np.zeros(max(cap_scored, 1), np.int32),
                 words=np.zeros(max(cap_scored, 1), np.int32), score=np.zeros(max(cap_scored, 1), np.float32),
                 acc=np.zeros(max(cap_scored, 1), np.float32))
        r = orb_kfdb_result(cap, ptr(b["cand"]), 0, cap_scored, ptr(b["id"]), ptr(b["words"]), ptr(b["score"]),
                            ptr(b["acc"]), 0, 0, 0, 0, 0.0)
        return r, b

    def _run(self, fn, name, queries, stages):
        """Call with room for 64 candidates / 256 scored keyframes per query; on ORB_E_CAPACITY the
        library has set the counts needed: call once more with those."""
        n = len(queries)
        caps = [(64, 256)] * n
        for attempt in range(2):
            res = [self._result(*c) for c in caps]
            qa = (orb_kfdb_query * max(n, 1))(*[q for q, _ in queries])
            ra = (orb_kfdb_result * max(n, 1))(*[r for r, _ in res])
            rc = fn(qa, ra, n)
            if rc == ORB_E_CAPACITY and attempt == 0:
                caps = [(max(ra[i].n_cand, 1), max(ra[i].n_scored, 1)) for i in range(n)]
                continue
            check(rc, name)
            break
        out = []
        for i in range(n):
            cand = res[i][1]["cand"][:ra[i].n_cand].copy()
            out.append((cand, KfdbStages(ra[i], res[i][1])) if stages else cand)
        return out

    def DetectLoopCandidates(self, bow: BowVector, connected_ids, minScore, stages=False):
        """vector<KeyFrame*> DetectLoopCandidates(KeyFrame* pKF, float minScore) (76-197):
        bow = pKF->mBowVec, connected_ids = pKF->GetConnectedKeyFrames()."""
        q = self._query(bow, connected_ids, minScore)
        return self._run(lambda qa, ra, n: self._L.KeyFrameDatabase_DetectLoopCandidates(self._h, qa, ra),
                         "KeyFrameDatabase_DetectLoopCandidates", [q], stages)[0]

    def DetectRelocalizationCandidates(self, bow: BowVector, stages=False):
        """vector<KeyFrame*> DetectRelocalizationCandidates(Frame* F) (199-309): bow = F->mBowVec."""
        q = self._query(bow)
        return self._run(lambda qa, ra, n: self._L.KeyFrameDatabase_DetectRelocalizationCandidates(self._h, qa, ra),
                         "KeyFrameDatabase_DetectRelocalizationCandidates", [q], stages)[0]

    def DetectRelocalizationCandidates_batch(self, bows, stages=False):
        """`len(bows)` frames against one database state in one launch set."""
        qs = [self._query(b) for b in bows]
        return self._run(
            lambda qa, ra, n: self._L.KeyFrameDatabase_DetectRelocalizationCandidates_batch(self._h, n, qa, ra),
            "KeyFrameDatabase_DetectRelocalizationCandidates_batch", qs, stages)


__all__ = ["KeyFrameDatabase", "KfdbStages", "OrbGpuError"]
