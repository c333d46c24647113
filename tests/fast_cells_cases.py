"""Cases that make every FAST corner of k_fast_cells visible in the extractor's output.

The extraction tests compare what the octree keeps, so a wrong score or a lost corner among the
culled ones is invisible to them.  Here the images and nfeatures are chosen so that the reference
keeps EVERY corner of every level (OracleExtractor(nf) and OracleExtractor(4 * nf) return the same
keypoints, i.e. no level's octree stops at its feature count, and the keypoints are as many as the
FAST corners, i.e. no two corners stay in one node), which turns the
keypoint list (position, response = FAST score), the descriptors and the corner count into a
check of every corner k_fast_cells writes.

Content (all seeded), chosen for the kernel's list, scoring and output code:
  dots    isolated pixels on a flat ground, each the only survivor of the pretest around it:
          survivor lists of length 0, 1, 2 and odd lengths (the pair scoring's neutral partner)
  blocks  8 x 8 blocks of 0 / 255 (with a jitter of 6): ring differences up to +-255 (the packed
          16-bit range), and lists longer than 512 entries, i.e. several 256-lane pair passes
  noise   flat ground + uniform noise of amplitude 9 (differences up to 18: between minTh 7 and
          iniTh 20) with isolated pixels in the left half: cells that fall back to minTh beside
          cells that keep their iniTh corners
  dense   a period-2 lattice of isolated extrema over the first cell: every second pixel of every
          second row is a corner and a strict local maximum, so the cell holds exactly
          ceil(dr / 2) * ceil(dc / 2) corners, its slot capacity (g.cap)
"""
import functools

import numpy as np

import extract_cases as ec
import oracle_lib

SF = 1.2
KOCT_NMAX = 640      # device octree node pool: nFeaturesPerLevel + 8 must fit

# (W, H, nlevels, nfeatures, kind).  185 x 125: level 0 has 5 x 3 cells of 31 x 31 (2 x 2, 1 x 2,
# 2 x 1 and 1 x 1 groups), level 1 (154 x 104) 4 x 2 cells of 31 x 36 (column pairs only), level 2
# (128 x 87) 3 x 1 cells.  122 x 100: 3 x 2 cells of 30 x 34 (a 2 x 2 group and a single column
# of two), level 1 (102 x 83) 2 x 1 cells of 35 x 51.
CASES = [
    (185, 125, 3, 900, "dots"),
    (122, 100, 2, 900, "blocks"),
    (185, 125, 3, 900, "noise"),
    (122, 100, 2, 900, "dense"),
]
BATCHES = [1, 3, 9]   # B >= 8 takes the XCD work order
# Seeds of a case's images 0 .. 8, picked on the CPU: the first ones for which the oracle's octree
# separates every corner (it stops early when a round of splits adds no node, so two close corners
# in an otherwise quiet image can stay in one node and one of them is dropped).
SEEDS = {"dots": [1, 2, 3, 4, 6, 7, 10, 11, 12], "blocks": [1, 2, 3, 4, 5, 6, 7, 8, 9],
         "noise": [1, 3, 4, 5, 6, 7, 8, 9, 10], "dense": [1, 2, 3, 4, 5, 6, 7, 8, 9]}


def case_id(c):
    return f"{c[4]}_{c[0]}x{c[1]}_l{c[2]}"


def _dots(rng, img, n, x1, sep=8):
    """n isolated pixels (one corner each, and the only survivor of the pretest around it) at
    least `sep` apart, left of column x1."""
    H, W = img.shape
    pts = []
    while len(pts) < n:
        y, x = int(rng.integers(17, H - 17)), int(rng.integers(17, x1 - 17))
        if all(max(abs(y - py), abs(x - px)) >= sep for py, px in pts):
            pts.append((y, x))
            img[y, x] = rng.choice([0, 30, 170, 255])
    return img


def generate(kind, W, H, seed):
    rng = np.random.default_rng(seed)
    if kind == "dots":
        return _dots(rng, np.full((H, W), 100, np.uint8), 8 + seed % 9, W)
    if kind == "blocks":
        # 0 / 255 with a jitter of 6 (below minTh: no corner inside a block) that breaks the
        # ties of equal scores, which the non-maximum suppression would otherwise all drop
        b = rng.integers(0, 2, ((H + 7) // 8, (W + 7) // 8), dtype=np.uint8)
        b = np.kron(b, np.ones((8, 8), np.uint8))[:H, :W].astype(bool)
        j = rng.integers(0, 7, (H, W))
        return np.where(b, 255 - j, j).astype(np.uint8)
    if kind == "noise":
        img = (128 + rng.integers(-9, 10, (H, W))).astype(np.uint8)
        return _dots(rng, img, 6, W // 2)
    if kind == "dense":
        # lattice pixels (19 + 2i, 19 + 2j), the first cell's detection pixels of even offset:
        # rows of i even 200, of i odd 50, everything else 125.  A lattice pixel's ring holds
        # only 125s and lattice pixels of the other row parity, so it is a corner of score 74;
        # every other pixel has a 125 in each arc of its ring and scores 0.
        img = np.full((H, W), 125, np.uint8)
        d = first_cell(W, H)
        for i in range((d[0] + 1) // 2):
            img[19 + 2 * i, 19:19 + d[1]:2] = 200 if i % 2 == 0 else 50
        img[int(rng.integers(60, H - 20)), int(rng.integers(70, W - 20))] = 255   # and one dot elsewhere
        return img
    raise ValueError(kind)


def image(kind, W, H, k=0):
    """Image k of a case's batch."""
    return generate(kind, W, H, SEEDS[kind][k])


def first_cell(W, H):
    """(detection rows, detection columns) of level 0's first cell."""
    p = ec.plan(W, H, SF, 1)[0]
    return p["hCell"], p["wCell"]


@functools.lru_cache(maxsize=None)
def reference(case, B):
    """-> (images [B, H, W], [(keypoints, descriptors)] of the oracle, corner total, complete).
    Computed once per (case, B) and shared; callers must not modify it."""
    W, H, nl, nf, kind = case
    imgs = np.stack([image(kind, W, H, k) for k in range(B)])
    orc, big = oracle_lib.OracleExtractor(nf, SF, nl, 20, 7), oracle_lib.OracleExtractor(4 * nf, SF, nl, 20, 7)
    res, total, complete = [], 0, True
    for b in range(B):
        k, d = orc(imgs[b])
        total += sum(len(orc.candidates(l)) for l in range(nl))
        kb, db = big(imgs[b])
        complete &= len(k) == len(kb) and np.array_equal(k.view(np.uint8), kb.view(np.uint8)) and np.array_equal(d, db)
        res.append((k, d))
    return imgs, res, total, complete


def fits_device(case):
    W, H, nl, nf, kind = case
    return int(oracle_lib.OracleExtractor(nf, SF, nl, 20, 7).tables()["n_per_level"].max()) + 8 <= KOCT_NMAX
