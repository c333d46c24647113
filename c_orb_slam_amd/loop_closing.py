"""Host-side mirror of the two steps of the reference's LoopClosing (src/LoopClosing.cc) that move the
map: the first half of CorrectLoop and the write-back of RunGlobalBundleAdjustment.  Both run in the HIP
library over the device-resident Map (c_orb_slam_amd.Map) and the caller's tables: the keyframe pose
table Tcw (n_kf_rows x 16 float32, indexed by mnId) and the map-point table (indexed by the map-point
row).

The tables are either numpy arrays (host pointers: copied up, corrected, copied back) or torch device
tensors (device pointers: corrected in place); a call takes all of one kind.  Every table argument is
changed in place where the call writes it."""
import ctypes as C

import numpy as np

from ._lib import check, lib, orb_gbaapply, orb_loopcorrect, orb_pointtable, ptr

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


__all__ = ["LoopClosing"]
