"""The cases of test_gpu_fast_cells.py reach what they are listed for (oracle only, no GPU)."""
import numpy as np
import pytest

import extract_cases as ec
import fast_cells_cases as fc


@pytest.mark.parametrize("B", fc.BATCHES, ids=lambda b: f"B{b}")
@pytest.mark.parametrize("case", fc.CASES, ids=fc.case_id)
def test_oracle_keeps_every_corner(case, B):
    imgs, ref, total, complete = fc.reference(case, B)
    assert complete
    assert fc.fits_device(case)
    assert sum(len(k) for k, _ in ref) == total
    assert total > 0


def test_geometry_reaches_every_group_shape():
    p = ec.plan(185, 125, fc.SF, 3)
    assert (p[0]["col_pairs"], p[0]["col_singles"], p[0]["row_pairs"], p[0]["row_singles"]) == (2, 1, 1, 1)
    assert p[1]["col_pairs"] == 2 and p[1]["row_pairs"] == 0
    q = ec.plan(122, 100, fc.SF, 2)
    assert (q[0]["col_pairs"], q[0]["col_singles"], q[0]["row_pairs"], q[0]["row_singles"]) == (1, 1, 1, 0)


def test_contents():
    """List lengths and branches the contents are meant to give, from the oracle's corners."""
    # dots: one corner (and one list entry) per dot; cells with 0, 1, 2 and an odd number >= 3
    imgs, ref, total, _ = fc.reference(fc.CASES[0], 9)
    per_cell = set()
    for k, _ in ref:
        l0 = k[k["octave"] == 0]
        cells, n = np.unique((l0["y"].astype(int) - 16) // 31 * 8 + (l0["x"].astype(int) - 16) // 31, return_counts=True)
        per_cell.update(n.tolist())
        assert len(cells) < 15
    assert {1, 2} <= per_cell and any(n % 2 for n in per_cell if n > 2), per_cell
    # blocks: both extremes next to each other, scores near the top of the range
    imgs, ref, total, _ = fc.reference(fc.CASES[1], 1)
    assert imgs.min() == 0 and imgs.max() == 255 and ref[0][0]["response"].max() >= 240.0
    # noise: corners below iniTh (cells that fell back to minTh) and corners above it
    imgs, ref, total, _ = fc.reference(fc.CASES[2], 1)
    r = ref[0][0][ref[0][0]["octave"] == 0]["response"]
    assert (r < 20).any() and (r >= 20).any(), (r.min(), r.max())
    # dense: the first cell holds exactly its slot capacity, ceil(dr / 2) * ceil(dc / 2) corners
    W, H, nl, nf, kind = fc.CASES[3]
    imgs, ref, total, _ = fc.reference(fc.CASES[3], 1)
    dr, dc = fc.first_cell(W, H)
    k0 = ref[0][0][ref[0][0]["octave"] == 0]
    first = k0[(k0["x"] < 19 + dc) & (k0["y"] < 19 + dr)]
    assert len(first) == ((dr + 1) // 2) * ((dc + 1) // 2), len(first)
    assert (first["response"] == 74.0).all()
