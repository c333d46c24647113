"""Every FAST corner of k_fast_cells against the CPU oracle (cases: fast_cells_cases.py).

For these images the reference's octree keeps every corner of every level, so keypoints (28
bytes, response = FAST score), descriptors and ORBextractor_last_corner_count must equal the
oracle's: a wrong score, a lost or a misplaced corner anywhere in a cell shows.  That the cases
have this property is asserted here with the oracle alone, and without a GPU in
test_fast_cells_cases_cpu.py.
"""
import pytest

import extract_cases as ec
import fast_cells_cases as fc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("B", fc.BATCHES, ids=lambda b: f"B{b}")
@pytest.mark.parametrize("case", fc.CASES, ids=fc.case_id)
def test_every_corner(gpu, case, B):
    W, H, nl, nf, kind = case
    imgs, ref, total, complete = fc.reference(case, B)
    assert complete, "the oracle's octree drops corners for this case: not a case for this test"
    ex = gpu.ORBextractor(nf, fc.SF, nl, 20, 7, max_width=W, max_height=H, max_batch=B)
    res = [ex(imgs[0])] if B == 1 else ex.extract_batch(imgs)
    assert ex.last_corner_count() == total, (ex.last_corner_count(), total)
    for b in range(B):
        ec.assert_keypoints_equal(res[b][0], res[b][1], ref[b][0], ref[b][1], nl, what=f"image {b}:")
    assert sum(len(r[0]) for r in ref) == total   # every corner is a keypoint
