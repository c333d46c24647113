"""Host-side mirror of the two steps of the reference's LoopClosing (src/LoopClosing.cc) that move the
map: the first half of CorrectLoop and the write-back of RunGlobalBundleAdjustment.  Both run in the HIP
library over the device-resident Map (c_orb_slam_amd.Map) and the caller's tables: the keyframe pose
table Tcw (n_kf_rows x 16 float32, indexed by mnId) and the map-point table (indexed by the map-point
row).

The tables are either numpy arrays (host pointers: copied up, corrected, copied back) or torch device
tensors (device pointers: corrected in place); a call takes all of one kind.  Every table argument is
changed in place where the call writes it.

SearchAndFuse is the loop fusion between the two (the "Start Loop Fusion" block of CorrectLoop and
LoopClosing::SearchAndFuse) over the same handle; it takes numpy tables only."""
import ctypes as C

import numpy as np

from ._lib import (ORB_E_CAPACITY, check, lib, orb_frame, orb_gbaapply, orb_loopcorrect, orb_loopfuse, orb_pointtable,
                   ptr)
from .map import CapacityError

_NP = {"f32": np.float32, "i32": np.int32, "u8": np.uint8}


class LoopClosing:
    def __init__(self, matcher, map):
        self._L, self._m, self._map = lib(), matcher, map

    # ---- pointer space
    @staticmethod
    def _on_device(a):
        return hasattr(a, "data_ptr")

    def _space(self, arrays):
        kinds = {self._on_device(a) for a in arrays if a is not None}
        if len(kinds) > 1:
            raise ValueError("the tables of one call are all numpy arrays or all torch device tensors")
        dev = kinds == {True}
        check(self._L.ORBmatcher_set_device_pointers(self._m._h, int(dev)))
        return dev

    @staticmethod
    def _p(a, kind, count):
        """The address of table array `a` after checking its type, size and layout."""
        if a is None:
            return None
        if LoopClosing._on_device(a):
            import torch
            want = {"f32": torch.float32, "i32": torch.int32, "u8": torch.uint8}[kind]
            if a.dtype != want or not a.is_contiguous() or a.numel() != count:
                raise ValueError(f"table array: expected {count} contiguous {kind}")
            return C.c_void_p(a.data_ptr()) if count else None
        if a.dtype != _NP[kind] or not a.flags.c_contiguous or a.size != count:
            raise ValueError(f"table array: expected {count} contiguous {kind}")
        return ptr(a) if count else None

    def _points(self, n, pos, normal, max_dist, min_dist, bad, ref_kf):
        return orb_pointtable(n, self._p(pos, "f32", 3 * n), self._p(normal, "f32", 3 * n),
                              self._p(max_dist, "f32", n), self._p(min_dist, "f32", n), self._p(bad, "u8", n),
                              self._p(ref_kf, "i32", n))

    @staticmethod
    def _rows(*arrays):
        """The row count of the table these arrays belong to (a missing one is the library's to reject)."""
        return max([int(a.shape[0]) for a in arrays if a is not None], default=0)

    def CorrectLoop(self, kf, cur_kf, Scw, scale_factors, Tcw, pos, normal, max_dist, min_dist, ref_kf,
                    corrected_ref, bad=None):
        """LoopClosing::CorrectLoop from CorrectedSim3[mpCurrentKF] = mg2oScw to the end of the loop over
        CorrectedSim3.  kf = mvpCurrentConnectedKFs with the current keyframe `cur_kf` (ids, any order);
        Scw = mg2oScw as 8 doubles (q xyzw, t, s); scale_factors = mvScaleFactors.  Tables, in place: Tcw
        (n_kf_rows x 16), pos / normal (n x 3), max_dist / min_dist (n), corrected_ref (n int32,
        mnCorrectedReference); read: ref_kf (n int32, mpRefKF's id or -1), bad (n uint8 or None).
        -> dict(CorrectedSim3, NonCorrectedSim3: nkf x 8 float64 in the order of kf, what
        OptimizeEssentialGraph takes; n_corrected; n_ref_missing)."""
        kf = np.ascontiguousarray(kf, np.int32)
        Scw = np.ascontiguousarray(Scw, np.float64).reshape(-1)
        sf = np.ascontiguousarray(scale_factors, np.float32)
        if Scw.size != 8:
            raise ValueError("Scw: 8 doubles (q xyzw, t, s)")
        self._space([Tcw, pos, normal, max_dist, min_dist, ref_kf, corrected_ref, bad])
        n, rows = self._rows(pos, normal, max_dist, min_dist, ref_kf, corrected_ref), self._rows(Tcw)
        cor, non = np.zeros((max(len(kf), 1), 8)), np.zeros((max(len(kf), 1), 8))
        c = orb_loopcorrect(len(kf), ptr(kf) if len(kf) else None, int(cur_kf), ptr(Scw), len(sf),
                            ptr(sf) if len(sf) else None, rows, self._p(Tcw, "f32", 16 * rows),
                            self._points(n, pos, normal, max_dist, min_dist, bad, ref_kf),
                            self._p(corrected_ref, "i32", n), ptr(cor), ptr(non), 0, 0)
        check(self._L.LoopClosing_CorrectLoop(self._m._h, self._map._h, C.byref(c)), "LoopClosing_CorrectLoop")
        return dict(CorrectedSim3=cor[:len(kf)], NonCorrectedSim3=non[:len(kf)], n_corrected=c.n_corrected,
                    n_ref_missing=c.n_ref_missing)

    def ApplyGlobalBA(self, origins, TcwGBA, kf_in_gba, Tcw, pos, posGBA, mp_in_gba, ref_kf, bad=None,
                      TcwBefGBA=None, kf_done=None):
        """The write-back of LoopClosing::RunGlobalBundleAdjustment: the spanning tree is walked from
        `origins` (mvpKeyFrameOrigins) over the map handle's children; keyframes outside the BA
        (kf_in_gba[id] == 0) take Tchild,parent * TcwGBA[parent]; every reached keyframe's Tcw becomes its
        TcwGBA (its old pose goes to TcwBefGBA when given, kf_done[id] = 1 when given); every point that is
        not bad takes posGBA (mp_in_gba) or is re-expressed through ref_kf.  Tables, in place: TcwGBA, Tcw,
        pos, TcwBefGBA, kf_done.  -> dict(n_kf_propagated, n_mp_gba, n_mp_moved, depth)."""
        origins = np.ascontiguousarray(origins, np.int32)
        self._space([TcwGBA, kf_in_gba, Tcw, pos, posGBA, mp_in_gba, ref_kf, bad, TcwBefGBA, kf_done])
        n, rows = self._rows(pos, posGBA, mp_in_gba, ref_kf), self._rows(Tcw, TcwGBA, kf_in_gba)
        g = orb_gbaapply(len(origins), ptr(origins) if len(origins) else None, rows, self._p(TcwGBA, "f32", 16 * rows),
                         self._p(kf_in_gba, "u8", rows), self._p(Tcw, "f32", 16 * rows),
                         self._points(n, pos, None, None, None, bad, ref_kf), self._p(posGBA, "f32", 3 * n),
                         self._p(mp_in_gba, "u8", n), self._p(TcwBefGBA, "f32", 16 * rows),
                         self._p(kf_done, "u8", rows), 0, 0, 0, 0)
        check(self._L.LoopClosing_ApplyGlobalBA(self._m._h, self._map._h, C.byref(g)), "LoopClosing_ApplyGlobalBA")
        return dict(n_kf_propagated=g.n_kf_propagated, n_mp_gba=g.n_mp_gba, n_mp_moved=g.n_mp_moved, depth=g.depth)

    def SearchAndFuse(self, kf, frames, Scw, loop_pts, kf_desc, table, logScaleFactor, cur_kf=-1, matched=None,
                      th=4.0, n_kf_rows=None, apply=True, cap_ops=4096, cap_updated=4096, retry=True):
        """The "Start Loop Fusion" block of LoopClosing::CorrectLoop and LoopClosing::SearchAndFuse: matched =
        mvpCurrentMatchedPoints (one id per slot of cur_kf's row, -1 = NULL; None skips that block) merged into
        the current keyframe, then one Fuse(pKF, Scw, mvpLoopMapPoints, th) with its Replaces per keyframe of
        kf (ids, any order; the passes run in ascending id), exact across the passes.  frames: their Frame
        objects; Scw: nkf x 8 float64 (q xyzw, t, s), the CorrectedSim3 of CorrectLoop; loop_pts =
        mvpLoopMapPoints as ids; kf_desc: mnId -> mDescriptors of every keyframe live in the handle (a dict
        or a list with None holes; n_kf_rows: the size of that table, default the largest id + 1); table:
        dict of the map-point table's numpy arrays pos, normal, max_dist, min_dist (read), desc, bad (written
        in place on success).  -> dict(nfused (nkf, the order of kf), ops (k x 6: pass, kind, a, b, kf, idx),
        updated, n_matched_skipped).  On ORB_E_CAPACITY the call is repeated once with the counts it
        reported (retry).  Numpy tables only: a matcher left in device-pointer mode (by a CorrectLoop over
        torch tensors) or deferred is refused with ORB_E_INVALID."""
        kf = np.ascontiguousarray(kf, np.int32)
        nkf = len(kf)
        Scw = np.ascontiguousarray(Scw, np.float64).reshape(-1, 8)
        if len(Scw) != nkf or len(frames) != nkf:
            raise ValueError("kf, frames and Scw: one entry per listed keyframe")
        loop = np.ascontiguousarray(loop_pts, np.int32)
        mt = None if matched is None else np.ascontiguousarray(matched, np.int32)
        items = list(kf_desc.items() if isinstance(kf_desc, dict) else enumerate(kf_desc))
        rows = {int(k): np.ascontiguousarray(d, np.uint8) for k, d in items if d is not None}
        nrows = int(n_kf_rows) if n_kf_rows is not None else max([k for k, _ in items], default=-1) + 1
        dptr = (C.c_void_p * max(nrows, 1))()
        for k, d in rows.items():
            if 0 <= k < nrows:
                dptr[k] = d.ctypes.data if d.size else None
        fr = (orb_frame * max(nkf, 1))()
        for k in range(nkf):
            fr[k] = frames[k].cstruct()
        want = dict(pos=np.float32, normal=np.float32, max_dist=np.float32, min_dist=np.float32, desc=np.uint8,
                    bad=np.uint8)
        for k, dt in want.items():
            a = table[k]
            if self._on_device(a) or a.dtype != dt or not a.flags.c_contiguous:
                raise ValueError(f"table[{k!r}]: a contiguous numpy array of {np.dtype(dt).name}")   # written in place
        n = len(table["bad"])
        nfused = np.zeros(max(nkf, 1), np.int32)
        caps = (int(cap_ops), int(cap_updated))
        for attempt in range(2):
            ops = np.zeros((max(caps[0], 1), 6), np.int32)
            upd = np.zeros(max(caps[1], 1), np.int32)
            f = orb_loopfuse(nkf, ptr(kf) if nkf else None, fr, ptr(Scw) if nkf else None, len(loop),
                             ptr(loop) if len(loop) else None, int(cur_kf), 0 if mt is None else len(mt),
                             None if mt is None else C.c_void_p(mt.ctypes.data), float(th), float(logScaleFactor),
                             nrows, C.cast(dptr, C.c_void_p), n, *(ptr(table[k]) if n else None for k in want),
                             int(apply), caps[0], caps[1], ptr(nfused), ptr(ops), ptr(upd), 0, 0, 0)
            rc = self._L.LoopClosing_SearchAndFuse(self._m._h, self._map._h, C.byref(f))
            if rc == ORB_E_CAPACITY and attempt == 0 and retry:
                caps = (max(f.n_ops, 1), max(f.n_updated, 1))
                continue
            if rc == ORB_E_CAPACITY:
                raise CapacityError(rc, "LoopClosing_SearchAndFuse", f.n_ops, f.n_updated)
            check(rc, "LoopClosing_SearchAndFuse")
            break
        return dict(nfused=nfused[:nkf].copy(), ops=ops[:f.n_ops].copy(), updated=upd[:f.n_updated].copy(),
                    n_matched_skipped=f.n_matched_skipped)

    def last_searchandfuse_timings(self):
        """ms of the last timed SearchAndFuse (Map.enable_timing): projection, match, descriptor recomputation
        (HIP events, summed over the passes) and the host replay (wall clock)."""
        ms = np.zeros(4, np.float32)
        check(self._L.LoopClosing_SearchAndFuse_last_timings(self._map._h, ptr(ms)),
              "LoopClosing_SearchAndFuse_last_timings")
        return ms


__all__ = ["LoopClosing"]
