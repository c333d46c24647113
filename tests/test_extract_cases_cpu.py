"""The extraction geometry table (extract_cases.py) on the CPU: every case runs in the oracle with
work on every level, plan() shows each feature a case is listed for, the threshold images are not
vacuous, and the rejected geometries fail in the oracle as well.  Editing a case so that a listed
feature is no longer reached fails here, without a GPU."""
import numpy as np
import pytest

import extract_cases as ec
import oracle_lib

PLANS = {c[:2]: ec.plan(*c[:4]) for c in ec.CASES}
ALL_LEVELS = [p for c in ec.CASES for p in PLANS[c[:2]]]


@pytest.mark.parametrize("case", ec.CASES, ids=ec.case_id)
def test_oracle_accepts_case_with_work_on_every_level(case):
    W, H, sf, nl, nf = case
    orc = oracle_lib.OracleExtractor(nf, sf, nl, 20, 7)
    k, d = orc(ec.image(W, H))
    per_level = [int((k["octave"] == l).sum()) for l in range(nl)]
    assert min(per_level) >= 5, per_level
    assert d.shape == (len(k), 32)
    # plan() restates the oracle's level sizes
    for p in PLANS[(W, H)]:
        assert orc.level(p["level"]).shape == (p["h"] + 2 * ec.EDGE, p["w"] + 2 * ec.EDGE)
        assert p["ok"] and p["fits"] and p["nIni"] >= 1


def test_table_one_level_one_cell():
    (p,) = PLANS[(62, 62)]
    assert (p["cols"], p["rows"], p["wCell"], p["hCell"]) == (1, 1, 30, 30)


def test_table_single_cell_levels():
    single = [p for p in ALL_LEVELS if p["cols"] == 1 and p["rows"] == 1]
    assert len(single) >= 5
    top = PLANS[(330, 250)][-1]
    assert (top["w"], top["h"], top["cols"], top["rows"], top["wCell"], top["hCell"]) == (82, 62, 1, 1, 50, 30)
    tail = PLANS[(240, 240)][11:]
    assert [(p["cols"], p["rows"]) for p in tail] == [(1, 1)] * 4
    assert tail[0]["wCell"] == 52 and tail[-1]["wCell"] == 31


def test_table_mixed_pairs_and_singles():
    P = PLANS[(160, 120)]
    assert any(p["col_pairs"] and p["col_singles"] for p in P)      # paired and single columns in one level
    assert any(p["row_pairs"] for p in P) and any(p["row_singles"] for p in P)
    assert (P[-1]["cols"], P[-1]["rows"]) == (2, 1)
    assert (PLANS[(320, 240)][-1]["cols"], PLANS[(320, 240)][-1]["rows"]) == (2, 1)
    # over the table: groups of 2 x 2, 2 x 1, 1 x 2 and 1 x 1 cells
    for want_c, want_r in ((1, 1), (1, 0), (0, 1), (0, 0)):
        assert any((p["col_pairs"] > 0) >= want_c and (p["row_pairs"] > 0) >= want_r and
                   (p["col_singles"] > 0) >= 1 - want_c and (p["row_singles"] > 0) >= 1 - want_r for p in ALL_LEVELS)


def test_table_tall_cells_and_widest_union():
    p = PLANS[(257, 129)][2]
    assert (p["w"], p["h"], p["wCell"], p["hCell"], p["rows"]) == (178, 90, 37, 58, 1)
    assert p["hCell"] == max(q["hCell"] for q in ALL_LEVELS)
    # a union ROI of exactly FC_MAXR rows and one of FC_MAXR columns
    assert max(q["roi_h"] for q in ALL_LEVELS) == ec.FC_MAXR
    assert max(q["roi_w"] for q in ALL_LEVELS) == ec.FC_MAXR


def test_table_initial_nodes():
    seen = {p["nIni"] for p in ALL_LEVELS}
    assert {1, 2, 3, 4, 6, 7} <= seen
    assert [p["nIni"] for p in PLANS[(257, 129)][2:]] == [3, 3, 3]
    assert [p["nIni"] for p in PLANS[(400, 94)]] == [6, 7, 7]


def test_table_strip_and_clipped_last_column():
    P = PLANS[(400, 94)]
    assert [p["rows"] for p in P[1:]] == [1, 1]
    assert P[1]["last_col"] == 22 and P[1]["last_col"] < P[1]["wCell"]
    assert PLANS[(333, 217)][0]["last_col"] == 22
    assert min(p["last_col"] for p in ALL_LEVELS) <= 12    # 780 x 200: 6 detection columns left


def test_table_scales_and_level_counts():
    assert {c[2] for c in ec.CASES} >= {1.1, 1.2, 1.5, 2.0, 3.0}
    assert sum(c[2] > 1.25 for c in ec.CASES) >= 3          # more than one staging round per resize tile
    assert max(c[3] for c in ec.CASES) == 15 and any(c[3] == 12 for c in ec.CASES) and any(c[3] == 1 for c in ec.CASES)
    # scale 3.0 at 780 wide: a full 32-row tile's source rectangle (rows x padded dword columns)
    # exceeds the 48 KB staging budget, so the 32-row variant has to shrink
    W, H, sf, nl, _ = next(c for c in ec.CASES if c[2] == 3.0)
    (w1, h1) = ec.level_sizes(W, H, sf, nl)[1]
    assert (w1, h1) == (260, 67)
    assert (32 * sf + 1) * (256 * sf) > 48 * 1024 > (16 * sf + 2) * (256 * sf + 8)
    assert w1 + 2 * ec.EDGE > 256                           # and the level is more than one tile wide
    assert [c[:2] for c in ec.BATCH8_CASES] == [(160, 120), (333, 217), (330, 250), (780, 200)]


def test_table_blur_tiles():
    # k_blur7 tiles are 128 x 32: levels narrower than one tile and shorter than two
    assert any(p["w"] < 128 and p["h"] < 64 for p in ALL_LEVELS)
    assert any(p["w"] % 128 and p["h"] % 32 for p in ALL_LEVELS)


def _extract(kind, th):
    _, _, sf, nl, nf = ec.THRESHOLD_GEOM
    return oracle_lib.OracleExtractor(nf, sf, nl, *th)(ec.threshold_image(kind))[0]


def test_threshold_images_are_not_vacuous():
    low = _extract("low_contrast", (20, 7))
    assert len(low) >= 50 and (low["response"] < 20).all()       # every keypoint comes from the minTh retry
    assert len(_extract("low_contrast", (20, 20))) == 0
    mix, mix20 = _extract("mixed", (20, 7)), _extract("mixed", (20, 20))
    assert len(mix) >= 300 and len(mix20) >= 300
    n_retry = int((mix["response"] < 20).sum())
    assert 0 < n_retry < len(mix) // 2                            # the retry decides some cells only
    assert (mix20["response"] >= 20).all()
    for kind in ("low_contrast", "mixed"):
        k = _extract(kind, (40, 0))
        assert len(k) >= 300 and k["response"].min() == 1         # a corner's score is never 0
        assert (k["response"] < 7).any()                          # minTh = 0 keeps what (20, 7) drops
    # iniTh < minTh: the retry can add nothing
    assert np.array_equal(_extract("low_contrast", (7, 20)).view(np.uint8), _extract("low_contrast", (7, 7)).view(np.uint8))
    assert len(_extract("noise", (255, 255))) == 0
    assert len(_extract("noise", (20, 7))) >= 400


@pytest.mark.parametrize("case", ec.REJECTED, ids=ec.case_id)
def test_rejected_geometries_fail_in_the_oracle(case):
    W, H, sf, nl, nf = case
    with pytest.raises(RuntimeError):
        oracle_lib.OracleExtractor(nf, sf, nl, 20, 7)(ec.image(W, H))


def test_rejected_geometries_are_what_they_claim():
    P = ec.plan(*ec.REJECTED[0][:4])
    assert (P[1]["w"], P[1]["h"]) == (81, 59) and P[0]["ok"] and not P[1]["ok"]
    P = ec.plan(*ec.REJECTED[1][:4])
    assert all(p["ok"] and p["fits"] for p in P) and [p["nIni"] for p in P] == [0, 0, 0]
