"""Geometry cases of the ORB extractor: the case table, its images, and the cell plan in plain Python.

The GPU extractor derives every launch from (W, H, scaleFactor, nlevels) in
Extractor::setup_geometry (csrc/orb_extract.hip).  The cases below are chosen for what that planner
and the kernels do with them; plan() restates the part of it that follows the reference
(ORBextractor.cc:776-829: the FAST cell grid) and the planner's own pairing of cells into 2 x 2
groups (spans()), so that tests/test_extract_cases_cpu.py can assert, without a GPU, that every case
still reaches what it is listed for.
"""
import math

import numpy as np

from c_orb_slam_amd import synthetic

EDGE = 19            # EDGE_THRESHOLD: the border of every padded level
FC_MAXR = 70         # k_fast_cells: most rows / columns of one staged (union) ROI
CELL_W = 30          # ORBextractor.cc:783

# (W, H, scaleFactor, nlevels, nfeatures)
CASES = [
    (62, 62, 1.2, 1, 50),        # one level, one 30 x 30 cell, no resize launch
    (160, 120, 1.2, 4, 300),     # paired and single rows / columns mixed; top level 2 x 1 cells
    (257, 129, 1.2, 5, 300),     # level 2 = 178 x 90: one row of cells 37 x 58, nIni 3 on levels 2-4
    (400, 94, 1.2, 3, 300),      # strip: nIni 6 and 7, one cell row, last column ROI 22 px
    (333, 217, 1.5, 4, 400),     # odd sizes, scale 1.5 (several staging rounds), last column ROI 22 px
    (330, 250, 2.0, 3, 400),     # scale 2.0; top level 82 x 62 = one 50 x 30 cell
    (320, 240, 1.1, 12, 500),    # 12 levels; top level 2 x 1 cells
    (240, 240, 1.1, 15, 500),    # 15 levels (the maximum); levels 11-14 single cells, 52 .. 31 px
    (780, 200, 3.0, 2, 400),     # scale 3.0: the 32-row resize tile must shrink; level 1 = 260 x 67
]
BATCH8_CASES = [c for c in CASES if (c[0], c[1]) in ((160, 120), (333, 217), (330, 250), (780, 200))]

# refused: the reference divides by zero / the octree has no initial node
REJECTED = [
    (97, 71, 1.2, 2, 200),       # level 1 = 81 x 59: nRows = 0
    (120, 230, 1.2, 3, 200),     # portrait: nIni = round(88 / 198) = 0
]

THRESHOLD_GEOM = (320, 240, 1.2, 4, 500)
THRESHOLDS = [(20, 7), (7, 20), (40, 0), (0, 0), (255, 255)]


def case_id(c):
    return f"{c[0]}x{c[1]}_s{c[2]}_l{c[3]}_n{c[4]}"


def image(W, H, k=0):
    """The case's image (k = 0), or the k-th other image of the same size."""
    return synthetic.textured_image(np.random.default_rng(W * 1000 + H + 7919 * k), W, H)


def noise(W, H, seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W), dtype=np.uint8)


def low_contrast(W, H, seed):
    t = synthetic.textured_image(np.random.default_rng(seed), W, H).astype(np.float64)
    return np.clip(np.rint(110.0 + 0.06 * (t - 110.0)), 0, 255).astype(np.uint8)


def mixed(W, H, seed):
    """Left half textured, right half low contrast: only some cells need the minTh retry."""
    t = synthetic.textured_image(np.random.default_rng(seed), W, H)
    out = low_contrast(W, H, seed)
    out[:, :W // 2] = t[:, :W // 2]
    return out


def threshold_image(kind, seed=5):
    W, H = THRESHOLD_GEOM[:2]
    return {"mixed": mixed, "low_contrast": low_contrast, "noise": noise}[kind](W, H, seed)


def level_sizes(W, H, sf, nl):
    """(w, h) per level: cvRound(W * mvInvScaleFactor[l]) in float, ORBextractor.cc:1109-1111."""
    sfd = float(np.float32(sf))
    scale = [np.float32(1.0)]
    for _ in range(1, nl):
        scale.append(np.float32(float(scale[-1]) * sfd))
    out = []
    for s in scale:
        inv = np.float32(1.0) / s
        out.append((int(np.rint(np.float32(W) * inv)), int(np.rint(np.float32(H) * inv))))
    return out


def _spans(a0, a1, b0, b1):
    """Two neighbouring ROIs [a0, a1), [b0, b1) share a workgroup (setup_geometry's spans())."""
    return a1 == b0 + 6 and b1 - b0 >= 7 and b1 - a0 <= FC_MAXR


def _axis(length):
    """One axis of a level's cell grid: -> None if the reference divides by zero, else a dict."""
    lo, hi = EDGE - 3, length - EDGE + 3
    extent = np.float32(hi - lo)
    n = int(extent / np.float32(CELL_W))
    if n <= 0:
        return None
    cell = int(math.ceil(float(extent / np.float32(n))))
    return dict(lo=lo, hi=hi, n=n, cell=cell)


def _rois(ax, skip_margin):
    """Kept cells' ROIs along one axis (rows skip at maxBorder - 3, columns at maxBorder - 6)."""
    out = []
    for i in range(ax["n"]):
        ini = ax["lo"] + i * ax["cell"]
        if ini >= ax["hi"] - skip_margin:
            continue
        out.append((ini, min(ini + ax["cell"] + 6, ax["hi"])))
    return out


def _pairing(rois):
    """-> (pairs, singles, extents of the unions) under the greedy left-to-right pairing."""
    pairs = singles = 0
    ext = []
    i = 0
    while i < len(rois):
        two = i + 1 < len(rois) and _spans(*rois[i], *rois[i + 1])
        ext.append(rois[i + 1 if two else i][1] - rois[i][0])
        pairs += two
        singles += not two
        i += 2 if two else 1
    return pairs, singles, ext


def plan(W, H, sf, nl):
    """Per level: size, cell grid, 2 x 2 grouping and the octree's initial node count.
    A level the reference cannot run (a cell count of 0) has ok = False and no grid."""
    out = []
    for l, (w, h) in enumerate(level_sizes(W, H, sf, nl)):
        ax, ay = _axis(w), _axis(h)
        d = dict(level=l, w=w, h=h, ok=ax is not None and ay is not None)
        if d["ok"]:
            cols, rows = _rois(ax, 6), _rois(ay, 3)
            cp, cs, cext = _pairing(cols)
            rp, rs, rext = _pairing(rows)
            d.update(nCols=ax["n"], nRows=ay["n"], wCell=ax["cell"], hCell=ay["cell"],
                     cols=len(cols), rows=len(rows), col_pairs=cp, col_singles=cs, row_pairs=rp, row_singles=rs,
                     last_col=cols[-1][1] - cols[-1][0], last_row=rows[-1][1] - rows[-1][0],
                     roi_w=max(cext), roi_h=max(rext),
                     fits=ax["cell"] + 6 <= FC_MAXR and ay["cell"] + 6 <= FC_MAXR)
            bw, bh = np.float32(ax["hi"] - ax["lo"]), np.float32(ay["hi"] - ay["lo"])
            d["nIni"] = int(math.floor(float(bw / bh) + 0.5))   # roundf, ORBextractor.cc:543
        out.append(d)
    return out


# ---- helpers of the GPU tests (test_gpu_extract_geometry.py, test_gpu_extract_paths.py)

PLAN_FLOW, PLAN_CHAIN, PLAN_FAST_SPLIT, PLAN_BLUR_SIDE, PLAN_BLUR_EARLY, PLAN_TILE32 = 1, 2, 4, 8, 16, 32


def extract_plan(ex):
    """orbgpu_debug_extract_plan of a c_orb_slam_amd.ORBextractor -> (flags, chain_from, tile_rows[2, nlevels])."""
    import ctypes as C
    from c_orb_slam_amd._lib import check, lib, ptr
    flags, chain_from = C.c_int(-1), C.c_int(-1)
    rows = np.zeros((2, ex.nlevels), np.int32)
    check(lib().orbgpu_debug_extract_plan(ex._h, C.byref(flags), C.byref(chain_from), ptr(rows)), "extract_plan")
    return flags.value, chain_from.value, rows


def diag(gk, ok, nl):
    msg = [f"gpu n={len(gk)} oracle n={len(ok)}"]
    for l in range(nl):
        a, b = gk[gk["octave"] == l], ok[ok["octave"] == l]
        if len(a) != len(b) or not np.array_equal(a.view(np.uint8), b.view(np.uint8)):
            msg.append(f" level {l}: gpu {len(a)} oracle {len(b)}")
            n = min(len(a), len(b))
            for f in ("x", "y", "angle", "response"):
                bad = np.nonzero(a[f][:n] != b[f][:n])[0]
                if len(bad):
                    i = bad[0]
                    msg.append(f"   first {f} mismatch at {i}: gpu {a[i]} oracle {b[i]}")
                    break
            break
    return "\n".join(msg)


def assert_levels_equal(ex, orc, nl, index=0, what=""):
    """Padded pyramid levels, then blurred levels, of image `index` of the last GPU call against
    the oracle's last image: the order that localises a divergence."""
    for l in range(nl):
        gl, ol = ex.image_pyramid_level(l, index), orc.level(l)
        assert gl.shape == ol.shape, f"{what} pyramid level {l}: shape {gl.shape} vs {ol.shape}"
        assert np.array_equal(gl, ol), f"{what} pyramid level {l} differs at {np.argwhere(gl != ol)[:5]}"
    for l in range(nl):
        gb, ob = ex.blurred_level(l, index), orc.blurred(l)
        assert gb.shape == ob.shape, f"{what} blurred level {l}: shape {gb.shape} vs {ob.shape}"
        assert np.array_equal(gb, ob), f"{what} blurred level {l} differs at {np.argwhere(gb != ob)[:5]}"


def assert_keypoints_equal(gk, gd, ok, od, nl, what=""):
    assert len(gk) == len(ok) and np.array_equal(gk.view(np.uint8), ok.view(np.uint8)), f"{what} {diag(gk, ok, nl)}"
    if len(ok):
        assert gd is not None and np.array_equal(gd, od), f"{what} descriptors differ at {np.argwhere(gd != od)[:5]}"
    else:
        assert gd is None or len(gd) == 0, what


def assert_extraction_equal(ex, orc, img, gk, gd, nl, index=0, what=""):
    """Everything the GPU extractor produced for `img` against a run of the oracle on it."""
    ok, od = orc(img)
    assert_levels_equal(ex, orc, nl, index, what)
    assert_keypoints_equal(gk, gd, ok, od, nl, what)
    return ok, od
