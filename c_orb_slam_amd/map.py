"""Host-side mirror of the part of the reference's Map / KeyFrame / MapPoint that relates keyframes
to map points (include/Map.h, src/KeyFrame.cc, src/MapPoint.cc): the rows live in device memory,
mutations go through the C ABI into a host mirror, and the two counting functions over the
relation -- KeyFrame::UpdateConnections here, Tracking::UpdateLocalMap as
ORBmatcher.UpdateLocalMap -- run in the HIP library.

Two rules hold everywhere: the vote reads only the slots whose observation exists (`observed`),
UpdateLocalPoints reads every slot; and ascending keyframe id stands in for the address order of
the reference's pointer-keyed std::map / std::set."""
import ctypes as C

import numpy as np

from ._lib import (ORB_E_CAPACITY, OrbGpuError, check, lib, orb_connections, orb_frame, orb_kfcull, orb_pointcull,
                   orb_searchneigh, ptr)


class CapacityError(OrbGpuError):
    """ORB_E_CAPACITY of SearchInNeighbors with the counts the call reported."""

    def __init__(self, code, what, n_ops, n_updated):
        super().__init__(code, what)
        self.n_ops, self.n_updated = n_ops, n_updated


class Map:
    def __init__(self):
        self._L = lib()
        h = C.c_void_p()
        check(self._L.Map_create(C.byref(h)), "Map_create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._L.Map_destroy(self._h)
            self._h = None

    __del__ = close

    def clear(self):
        check(self._L.Map_clear(self._h), "Map_clear")

    def size(self):
        """(live keyframes, slots of their rows, observed slots among them)"""
        n, s, o = C.c_int(), C.c_longlong(), C.c_longlong()
        check(self._L.Map_size(self._h, C.byref(n), C.byref(s), C.byref(o)), "Map_size")
        return n.value, s.value, o.value

    def AddKeyFrame(self, id, mp, observed=None):
        """Map::AddKeyFrame with the keyframe's mvpMapPoints (ids, -1 = none); observed[slot] = the
        point's mObservations holds (keyframe, slot) (None: all)."""
        mp = np.ascontiguousarray(mp, np.int32)
        ob = None if observed is None else np.ascontiguousarray(observed, np.uint8)
        check(self._L.Map_AddKeyFrame(self._h, int(id), len(mp), ptr(mp) if len(mp) else None,
                                      ptr(ob) if ob is not None and len(ob) else None), "Map_AddKeyFrame")

    def SetMapPointMatches(self, id, slots, mp, observed=None):
        """KeyFrame::AddMapPoint / EraseMapPointMatch / ReplaceMapPointMatch and MapPoint::AddObservation /
        EraseObservation: slot slots[k] of keyframe `id` takes mp[k] (-1 empties it) with observed[k]."""
        sl = np.ascontiguousarray(slots, np.int32)
        mp = np.ascontiguousarray(mp, np.int32)
        ob = None if observed is None else np.ascontiguousarray(observed, np.uint8)
        check(self._L.Map_SetMapPointMatches(self._h, int(id), len(sl), ptr(sl) if len(sl) else None,
                                             ptr(mp) if len(sl) else None,
                                             ptr(ob) if ob is not None and len(ob) else None),
              "Map_SetMapPointMatches")

    def EraseMapPoint(self, mp):
        """MapPoint::SetBadFlag"""
        check(self._L.Map_EraseMapPoint(self._h, int(mp)), "Map_EraseMapPoint")

    def ReplaceMapPoint(self, mp, by):
        """MapPoint::Replace"""
        check(self._L.Map_ReplaceMapPoint(self._h, int(mp), int(by)), "Map_ReplaceMapPoint")

    def EraseKeyFrame(self, id):
        """KeyFrame::SetBadFlag"""
        check(self._L.Map_EraseKeyFrame(self._h, int(id)), "Map_EraseKeyFrame")

    def SetNeighbours(self, id, best10, parent=-1, children=()):
        """GetBestCovisibilityKeyFrames(10), GetParent and GetChilds of keyframe `id` as ids."""
        b = np.ascontiguousarray(best10, np.int32)
        c = np.ascontiguousarray(children, np.int32)
        check(self._L.Map_SetNeighbours(self._h, int(id), len(b), ptr(b) if len(b) else None, int(parent), len(c),
                                        ptr(c) if len(c) else None), "Map_SetNeighbours")

    def UpdateConnections_batch(self, ids, cap_counter=256, cap_ordered=64):
        """KeyFrame::UpdateConnections of every keyframe of `ids` against one map state.  -> per
        keyframe (counter_id, counter_n, ordered_id, ordered_w): KFcounter in ascending id, and
        mvpOrderedConnectedKeyFrames / mvOrderedWeights.  On ORB_E_CAPACITY the call is repeated
        once with the counts it reported."""
        ids = np.ascontiguousarray(ids, np.int32)
        n = len(ids)
        caps = [(int(cap_counter), int(cap_ordered))] * n
        for attempt in range(2):
            bufs = [tuple(np.zeros(max(c, 1), np.int32) for c in (cc, cc, co, co)) for cc, co in caps]
            ra = (orb_connections * max(n, 1))()
            for i in range(n):
                r, b = ra[i], bufs[i]
                r.cap_counter, r.cap_ordered = caps[i]
                r.counter_id, r.counter_n, r.ordered_id, r.ordered_w = (ptr(x) for x in b)
            rc = self._L.KeyFrame_UpdateConnections_batch(self._h, n, ptr(ids) if n else None, ra)
            if rc == ORB_E_CAPACITY and attempt == 0:
                caps = [(max(ra[i].n_counter, 1), max(ra[i].n_ordered, 1)) for i in range(n)]
                continue
            check(rc, "KeyFrame_UpdateConnections_batch")
            break
        return [(b[0][:ra[i].n_counter].copy(), b[1][:ra[i].n_counter].copy(), b[2][:ra[i].n_ordered].copy(),
                 b[3][:ra[i].n_ordered].copy()) for i, b in enumerate(bufs)]

    def UpdateConnections(self, id, **kw):
        return self.UpdateConnections_batch([id], **kw)[0]

    def SetKeyFrameKeys(self, id, octave, uRight=None, depth=None, thDepth=0.0):
        """The per-slot key attributes of keyframe `id` (the KeyFrame constructor): octave =
        mvKeysUn[i].octave, uRight = mvuRight (None: monocular), depth = mvDepth with thDepth = mThDepth
        (None: no slot is far)."""
        oc = np.ascontiguousarray(octave, np.uint8)
        ur = None if uRight is None else np.ascontiguousarray(uRight, np.float32)
        de = None if depth is None else np.ascontiguousarray(depth, np.float32)
        check(self._L.Map_SetKeyFrameKeys(self._h, int(id), len(oc), ptr(oc) if len(oc) else None,
                                          ptr(ur) if ur is not None and len(ur) else None,
                                          ptr(de) if de is not None and len(de) else None, float(thDepth)),
              "Map_SetKeyFrameKeys")

    def KeyFrameCulling(self, cand, not_erase=None, monocular=False, bad=None, apply=True, cap_bad=64):
        """LocalMapping::KeyFrameCulling over cand = GetVectorCovisibleKeyFrames() as ids.  -> dict(nMPs,
        nRedundant, verdict (0 kept, 1 SetBadFlag, 2 mbToBeErased, 3 skipped), bad_mp = the points that went
        bad through the culls).  apply: the handle erases the culled keyframes and those points.  On
        ORB_E_CAPACITY the call is repeated once with the count it reported."""
        cand = np.ascontiguousarray(cand, np.int32)
        n = len(cand)
        ne = None if not_erase is None else np.ascontiguousarray(not_erase, np.uint8)
        b = None if bad is None else np.ascontiguousarray(bad, np.uint8)
        nmps, nred, ver = (np.zeros(max(n, 1), np.int32) for _ in range(3))
        cap = int(cap_bad)
        for attempt in range(2):
            bmp = np.zeros(max(cap, 1), np.int32)
            r = orb_kfcull(n, ptr(cand) if n else None, ptr(ne) if ne is not None and n else None, int(monocular),
                           ptr(b) if b is not None and len(b) else None, 0 if b is None else len(b), cap, int(apply),
                           ptr(nmps), ptr(nred), ptr(ver), ptr(bmp), 0)
            rc = self._L.LocalMapping_KeyFrameCulling(self._h, C.byref(r))
            if rc == ORB_E_CAPACITY and attempt == 0:
                cap = r.n_bad
                continue
            check(rc, "LocalMapping_KeyFrameCulling")
            break
        return dict(nMPs=nmps[:n].copy(), nRedundant=nred[:n].copy(), verdict=ver[:n].copy(),
                    bad_mp=bmp[:r.n_bad].copy())

    def MapPointCulling(self, mp, first_kf, found, visible, cur_kf, monocular=False, bad=None, apply=True):
        """LocalMapping::MapPointCulling over mlpRecentAddedMapPoints as ids with their mnFirstKFid, mnFound and
        mnVisible.  -> (verdict, observations): 0 keep, 1 dropped (already bad), 2 bad by found ratio, 3 bad
        by observations, 4 dropped (old enough).  apply: the handle erases the points with verdict 2 or 3."""
        a = [np.ascontiguousarray(x, np.int32) for x in (mp, first_kf, found, visible)]
        n = len(a[0])
        b = None if bad is None else np.ascontiguousarray(bad, np.uint8)
        ver, ob = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
        r = orb_pointcull(n, *(ptr(x) if n else None for x in a), ptr(b) if b is not None and len(b) else None,
                          0 if b is None else len(b), int(cur_kf), int(monocular), int(apply), ptr(ver), ptr(ob))
        check(self._L.LocalMapping_MapPointCulling(self._h, C.byref(r)), "LocalMapping_MapPointCulling")
        return ver[:n].copy(), ob[:n].copy()

    def SearchInNeighbors(self, matcher, cur_kf, cur, target_ids, targets, kf_desc, Ow, scale_factors, table,
                          logScaleFactor, th=3.0, apply=True, cap_ops=4096, cap_updated=4096, retry=True):
        """LocalMapping::SearchInNeighbors (LocalMapping.cc:454-553): every Fuse pass into the targets, the
        backward pass into the current keyframe and the update of its points, exact across the passes.
        cur / targets: Frame objects of mpCurrentKeyFrame and vpTargetKFs (ids cur_kf / target_ids, the
        reference's order); kf_desc: mnId -> mDescriptors of every keyframe live in the handle (a dict or a
        list with None holes); Ow: n_kf_rows x 3 camera centres by mnId; table: dict of the map-point table's
        arrays pos, desc, normal, max_dist, min_dist, bad, ref_kf with rows = map-point ids (desc, normal,
        max_dist, min_dist and bad are written in place on success).  -> dict(nfused (ntargets + 1), ops
        (k x 6: pass, kind, a, b, kf, idx), updated, n_ref_missing).  On ORB_E_CAPACITY the call is repeated
        once with the counts it reported (retry)."""
        Ow = np.ascontiguousarray(Ow, np.float32).reshape(-1, 3)
        nrows = len(Ow)
        items = kf_desc.items() if isinstance(kf_desc, dict) else enumerate(kf_desc)
        rows = {int(k): np.ascontiguousarray(d, np.uint8) for k, d in items if d is not None}
        dptr = (C.c_void_p * max(nrows, 1))()
        for k, d in rows.items():
            if 0 <= k < nrows:
                dptr[k] = d.ctypes.data if d.size else None
        tid = np.ascontiguousarray(target_ids, np.int32)
        nt = len(tid)
        fr = (orb_frame * max(nt, 1))()
        for t in range(nt):
            fr[t] = targets[t].cstruct()
        fc = cur.cstruct()
        sf = np.ascontiguousarray(scale_factors, np.float32)
        want = dict(pos=np.float32, desc=np.uint8, normal=np.float32, max_dist=np.float32, min_dist=np.float32,
                    bad=np.uint8, ref_kf=np.int32)
        for k, dt in want.items():
            a = table[k]
            assert a.dtype == dt and a.flags["C_CONTIGUOUS"], k   # written in place
        n = len(table["bad"])
        nfused = np.zeros(nt + 1, np.int32)
        caps = (int(cap_ops), int(cap_updated))
        for attempt in range(2):
            ops = np.zeros((max(caps[0], 1), 6), np.int32)
            upd = np.zeros(max(caps[1], 1), np.int32)
            S = orb_searchneigh(int(cur_kf), C.pointer(fc), nt, ptr(tid) if nt else None, fr, float(th),
                                float(logScaleFactor), nrows, C.cast(dptr, C.c_void_p), ptr(Ow) if nrows else None,
                                len(sf), ptr(sf), n, *(ptr(table[k]) if n else None for k in want), int(apply),
                                caps[0], caps[1], ptr(nfused), ptr(ops), ptr(upd), 0, 0, 0)
            rc = self._L.LocalMapping_SearchInNeighbors(matcher._h, self._h, C.byref(S))
            if rc == ORB_E_CAPACITY and attempt == 0 and retry:
                caps = (max(S.n_ops, 1), max(S.n_updated, 1))
                continue
            if rc == ORB_E_CAPACITY:
                raise CapacityError(rc, "LocalMapping_SearchInNeighbors", S.n_ops, S.n_updated)
            check(rc, "LocalMapping_SearchInNeighbors")
            break
        return dict(nfused=nfused, ops=ops[:S.n_ops].copy(), updated=upd[:S.n_updated].copy(),
                    n_ref_missing=S.n_ref_missing)

    def last_searchneigh_timings(self):
        """ms of the last timed SearchInNeighbors (enable_timing): projection, match, descriptor recomputation,
        final update (HIP events, summed over the passes) and the host replay (wall clock)."""
        ms = np.zeros(5, np.float32)
        check(self._L.LocalMapping_SearchInNeighbors_last_timings(self._h, ptr(ms)),
              "LocalMapping_SearchInNeighbors_last_timings")
        return ms

    def enable_timing(self, on=True):
        check(self._L.Map_enable_timing(self._h, int(on)), "Map_enable_timing")

    def last_timings(self):
        """ms of the last timed UpdateLocalMap: (index rebuild or -1, vote, keyframe selection, local
        points, remap + gather), HIP events."""
        ms = np.zeros(5, np.float32)
        check(self._L.Map_last_timings(self._h, ptr(ms)), "Map_last_timings")
        return ms


__all__ = ["Map", "OrbGpuError"]
