"""Seeded generators for the Map tests: lists of mutation calls that a test applies to the library's
Map and to the restatement (tests/map_ref.py) alike, and frames (lists of map-point ids) to query."""
import numpy as np


def apply(target, ops):
    """Every op is (method name, args...); RefMap and c_orb_slam_amd.Map share the names."""
    for op in ops:
        getattr(target, op[0])(*op[1:])


def gen_map(seed, n_kf, row, n_pts, fill=0.8, p_unobserved=0.05, hot=0, id_step=1):
    """n_kf keyframes (ids k * id_step) with rows of `row` slots over points [0, n_pts * 3 / 4): keyframe k
    sees a window of the point range around its own place, so that neighbouring keyframes share points;
    the last quarter of the ids is never held.  hot > 0: point 0 sits in the first `hot` rows (a point with
    many observations).  -> ops (AddKeyFrame only)"""
    rng = np.random.default_rng(seed)
    used = max(n_pts * 3 // 4, row + 1)
    ops = []
    for k in range(n_kf):
        centre = int(k * used / max(n_kf, 1))
        cand = (centre + np.arange(-row, row)) % used
        if hot:
            cand = cand[cand != 0]
        cand = np.unique(cand)
        take = rng.permutation(cand)[:min(int(row * fill), len(cand))]
        mp = np.full(row, -1, np.int32)
        where = rng.permutation(row)[:len(take)]
        mp[where] = take
        if hot and k < hot:
            mp[where[0]] = 0
        obs = (rng.random(row) >= p_unobserved).astype(np.uint8)
        ops.append(("AddKeyFrame", k * id_step, mp, obs))
    return ops


def gen_neighbours(seed, ref, extra_ids=()):
    """SetNeighbours for every live keyframe of `ref`: best10 from its own UpdateConnections, a random older
    parent, the children that follow from the parents; extra_ids (erased / unknown ids) are mixed into the lists."""
    rng = np.random.default_rng(seed)
    live = sorted(k for k, kf in ref.kfs.items() if not kf.isBad())
    parent = {}
    for i, k in enumerate(live):
        parent[k] = int(live[rng.integers(0, i)]) if i and rng.random() < 0.9 else -1
    children = {k: [] for k in live}
    for k, p in parent.items():
        if p >= 0:
            children[p].append(k)
    ops = []
    for k in live:
        best = list(ref.UpdateConnections(k)[2][:10])
        ch = list(children[k])
        par = parent[k]
        if len(extra_ids):
            if rng.random() < 0.5:
                best.insert(int(rng.integers(0, len(best) + 1)), int(rng.choice(extra_ids)))
                best = best[:10]
            if rng.random() < 0.3:
                ch.append(int(rng.choice(extra_ids)))
            if rng.random() < 0.1:
                par = int(rng.choice(extra_ids))
        ops.append(("SetNeighbours", k, np.array(best, np.int32), par, np.array(sorted(set(ch)), np.int32)))
    return ops


def gen_frames(seed, ref, count, N, n_pts, p_dup=0.05, p_none=0.2, p_stray=0.05):
    """`count` frames of N keypoints: most hold points of one or two random live keyframes' rows, some hold
    nothing (-1), some a point twice, some a never-observed id."""
    rng = np.random.default_rng(seed)
    live = sorted(k for k, kf in ref.kfs.items() if not kf.isBad())
    out = []
    for _ in range(count):
        pool = []
        for k in rng.choice(live, size=min(2, len(live)), replace=False):
            pool += [m.mnId for m in ref.kfs[int(k)].mvpMapPoints if m is not None]
        pool = np.unique(np.array(pool if pool else [0], np.int64))
        f = np.full(N, -1, np.int32)
        n_take = min(len(pool), int(N * (1 - p_none)))
        f[:n_take] = rng.permutation(pool)[:n_take]
        nd = int(N * p_dup)
        if n_take:
            f[n_take:n_take + nd] = rng.choice(f[:n_take], nd)
        ns = int(N * p_stray)
        f[N - ns:] = rng.integers(n_pts * 3 // 4, n_pts, ns)
        out.append(rng.permutation(f).astype(np.int32))
    return out
