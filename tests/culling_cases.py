"""Seeded generators for the culling tests: lists of mutation calls (applied to the library's Map and to
tests/culling_ref.py alike, as in map_cases.py) and the culling calls to make on the result.  Rows hold at most a
few hundred slots and maps 3-150 keyframes."""
import numpy as np

TH_DEPTH = 40.0


def keys(rng, n, stereo, spread=0.15):
    """SetKeyFrameKeys arguments of a row of n slots: octaves mostly 0-2, a few higher; for a stereo sensor about
    two thirds of the slots have a right coordinate, and those a depth on either side of TH_DEPTH."""
    octave = rng.integers(0, 3, n) + (rng.random(n) < spread) * rng.integers(2, 6, n)
    if not stereo:
        return octave.astype(np.uint8), None, None, 0.0
    has = rng.random(n) < 0.67
    uRight = np.where(has, rng.random(n) * 600.0, -1.0).astype(np.float32)
    depth = np.where(has, 0.5 + rng.random(n) * 45.0, -1.0).astype(np.float32)
    return octave.astype(np.uint8), uRight, depth, TH_DEPTH


def gen_cull_map(seed, n_kf, row, span, step, fill=0.9, stereo=False, p_unobserved=0.03, first_id=0, first_pt=0,
                 spread=0.15):
    """n_kf keyframes (ids first_id ..) of `row` slots: keyframe k holds a share `fill` of the points
    [first_pt + k * step, first_pt + k * step + span), so a point has about span / step * fill holders.
    -> ops (AddKeyFrame + SetKeyFrameKeys per keyframe)"""
    rng = np.random.default_rng(seed)
    assert span <= row
    ops = []
    for k in range(n_kf):
        window = first_pt + k * step + np.arange(span)
        take = window[rng.random(span) < fill]
        mp = np.full(row, -1, np.int32)
        mp[rng.permutation(row)[:len(take)]] = take
        obs = (rng.random(row) >= p_unobserved).astype(np.uint8)
        ops.append(("AddKeyFrame", first_id + k, mp, obs))
        ops.append(("SetKeyFrameKeys", first_id + k) + keys(rng, row, stereo, spread))
    return ops


def gadget_break(first_id, first_pt):
    """Four keyframes over the same 10 points, octave 0, monocular: culling the first leaves the second with
    two other observers per point.  candidates [a, a + 1] -> verdicts [1, 0]."""
    pts = first_pt + np.arange(10, dtype=np.int32)
    ops = []
    for k in range(4):
        ops.append(("AddKeyFrame", first_id + k, pts.copy(), None))
        ops.append(("SetKeyFrameKeys", first_id + k, np.zeros(10, np.uint8), None, None, 0.0))
    return ops, [first_id, first_id + 1]


def gadget_create(first_id, first_pt):
    """A = first_id holds 19 points shared with three helpers and 2 shared with B = first_id + 1 and one helper
    only; B holds those 2 and 10 points shared with the helpers.  B alone counts 10 of 12 and stays; once A is
    culled the 2 points fall to two observations and go bad, B counts 10 of 10 and goes.  candidates [A, B]"""
    a_pts = first_pt + np.arange(19)
    two = first_pt + 19 + np.arange(2)
    b_pts = first_pt + 21 + np.arange(10)
    rows = [np.concatenate([a_pts, two]), np.concatenate([two, b_pts]), np.concatenate([a_pts, two, b_pts]),
            np.concatenate([a_pts, b_pts]), np.concatenate([b_pts, a_pts])]
    ops = []
    for k, r in enumerate(rows):
        ops.append(("AddKeyFrame", first_id + k, r.astype(np.int32), None))
        ops.append(("SetKeyFrameKeys", first_id + k, np.zeros(len(r), np.uint8), None, None, 0.0))
    return ops, [first_id, first_id + 1]


# name: (seed, n_kf, row, span, step, fill, stereo sensor, spread, gadgets)
FAMILIES = {
    "dense_mono": (1, 40, 200, 160, 16, 0.95, False, 0.1, True),
    "dense_stereo": (2, 40, 200, 160, 16, 0.95, True, 0.1, True),
    "sparse_mono": (3, 30, 128, 100, 60, 0.8, False, 0.15, False),
    "three_keyframes": (4, 3, 64, 60, 2, 1.0, False, 0.0, False),
    "many_keyframes": (5, 150, 96, 90, 6, 0.9, True, 0.2, True),
}


def family(name):
    """-> (ops, calls, n_pts): calls = [(cand, not_erase or None, monocular)], to be made one after another, each
    applied before the next; n_pts bounds every point id."""
    seed, n_kf, row, span, step, fill, stereo, spread, gadgets = FAMILIES[name]
    rng = np.random.default_rng(1000 + seed)
    ops = gen_cull_map(seed, n_kf, row, span, step, fill, stereo, spread=spread)
    n_pts = n_kf * step + span
    extra = []
    if gadgets:
        g1, c1 = gadget_break(n_kf, n_pts)
        g2, c2 = gadget_create(n_kf + 4, n_pts + 10)
        ops += g1 + g2
        n_pts += 10 + 31
        extra = [c2, c1]
    calls = []
    for cur in rng.permutation(n_kf)[:3]:
        # the covisibles of a keyframe: its neighbours in id, nearest first, then the gadgets' candidates
        near = [int(cur) + d for d in (1, -1, 2, -2, 3, -3, 4, -4, 5, -5, 6) if 0 <= cur + d < n_kf]
        cand = near + [k for c in extra for k in c]
        extra = []
        ne = (rng.random(len(cand)) < 0.25).astype(np.uint8)
        ne[len(near):] = 0
        calls.append((np.array(cand, np.int32), ne if rng.random() < 0.7 else None, not stereo))
    return ops, calls, n_pts + 8


def gen_point_lists(seed, n_pts, n, cur_kf):
    """MapPointCulling arguments over ids [0, n_pts) without repeats: found / visible around the 0.25 threshold,
    first keyframes 0-4 before cur_kf."""
    rng = np.random.default_rng(seed)
    mp = rng.permutation(n_pts)[:n].astype(np.int32)
    visible = rng.integers(1, 40, len(mp)).astype(np.int32)
    found = np.minimum(visible, (visible * rng.choice([0.1, 0.25, 0.3, 1.0], len(mp)))).astype(np.int32)
    found[::7] = visible[::7] // 4                                          # at or just below a quarter
    first = (cur_kf - rng.integers(0, 5, len(mp))).astype(np.int32)
    return mp, first, found, visible
