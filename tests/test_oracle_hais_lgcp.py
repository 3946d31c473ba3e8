"""The cases of tests/hais_lgcp_cases.py on the CPU, from the restatement alone: each case is what its row says, every loss
is finite, and the restatement's float32-against-float64 gap — the reference of the bars tests/test_gpu_hais_lgcp.py holds the HIP
path to — is the stored one (tests/golden/hais_lgcp_gaps.json): re-measured, held to 1.5 x the stored value and never above a
quarter of the bar it sets.  The float32 run takes at most 8 threads (lgcp_grad_cases.run_restatement says why)."""
import numpy as np
import pytest
import torch

import hais_lgcp_cases as hc
import hais_restatement as hr
from cmcd_amd import synthetic

ROWS = {  # id: (n, K, L, eps, eta, ngrid + 1, row blocks as (rows, second half))
    "n1": (1, 2, 2, 0.02, 0.6, 3, [(1, False)]),
    "n16": (16, 2, 2, 0.02, 0.6, 3, [(16, False)]),
    "n17": (17, 2, 2, 0.02, 0.6, 3, [(17, True)]),
    "n32": (32, 2, 2, 0.02, 0.6, 3, [(32, True)]),
    "n33": (33, 2, 2, 0.02, 0.6, 3, [(32, True), (1, False)]),
    "n65": (65, 2, 2, 0.02, 0.6, 3, [(32, True), (32, True), (1, False)]),
    "k1l1": (20, 1, 1, 0.02, 0.6, 2, [(20, True)]),
    "l3": (20, 2, 3, 0.05, 0.6, 3, [(20, True)]),
    "offgrid": (20, 3, 1, 0.02, 0.6, 6, [(20, True)]),
    "k5grid2": (20, 5, 1, 0.1, 0.3, 3, [(20, True)]),
    "eta0": (20, 2, 2, 0.02, 0.0, 3, [(20, True)]),
    "big": (20, 3, 3, 0.2, 0.6, 4, [(20, True)]),
    "refdefault": (20, 2, 1, 1e-5, 0.0, 3, [(20, True)]),
}


def test_the_table_and_the_cases_agree():
    assert sorted(ROWS) == sorted(hc.IDS) and len(hc.IDS) == 13
    assert hc.GRAD_IDS == [i for i in hc.IDS if i != "refdefault"]
    assert (hc.ROW_BLOCK, hc.HALF, hc.COL_TILE) == (32, 16, 16) and 64 % hc.COL_TILE == 0 and hc.D % 64 == 0
    assert abs(hc.MU0 - 3.88) < 5e-3
    assert sorted(hc.stored_gaps()) == sorted(hc.IDS)


@pytest.mark.parametrize("cid", hc.IDS)
def test_case_is_what_its_row_says(cid):
    case = hc.case_by_id(cid)
    n, K, L, eps, eta, ny, rbs = ROWS[cid]
    flat, un, fixed = hc.params(case)
    p = hr.params_numpy(un, flat)
    assert fixed == (hc.D, K, L) and len(hc.seeds_of(case)) == n and hc.row_blocks(n) == rbs
    assert np.array_equal(hc.seeds_of(case), synthetic.parity_seeds(n))
    assert p["eps"] == np.float32(eps) and p["eta"] == np.float32(eta)
    assert p["mgridref_y"].shape == (ny,) and len(set(p["mgridref_y"].tolist())) == ny          # non-uniform
    assert p["vd"]["mean"].shape == (hc.D,) and abs(p["vd"]["mean"].mean() - hc.MU0) < 0.1 and p["vd"]["mean"].std() > 0.5
    sigma = case[7]
    assert abs(np.exp(p["vd"]["logdiag"].mean()) - sigma) < 0.05 * sigma and p["vd"]["logdiag"].std() > 0.1
    assert p["md"].std() > 0.1
    frac, _ = hr.fractions(K, ny - 1)
    on_nodes = np.allclose(frac, np.round(frac))
    assert on_nodes == (cid not in ("offgrid", "k5grid2")), (cid, frac)
    l, z, g = hc.reference(case)
    assert l.shape == (n,) and z.shape == (n, hc.D) and np.isfinite(l).all() and np.isfinite(z).all()
    if cid == "refdefault":
        assert g is None and not case[8]
        return
    names = [name for name, _ in hc.blocks(g)]
    assert len(names) == 3 * 26 + 2 + ny and 82 <= len(names) <= 86 and len(set(names)) == len(names)
    for name, a in hc.blocks(g):
        assert np.isfinite(a).all() and np.abs(a).max() > 0.0, name     # every block of every case carries a gradient
    if cid == "eta0":
        assert abs(g[("eta",)]) > 0.0                                  # d / d eta does not vanish at eta = 0


@pytest.mark.parametrize("cid", hc.IDS)
def test_float32_gap_is_the_stored_one(cid):
    case = hc.case_by_id(cid)
    assert torch.get_num_threads() >= 1
    got, stored = hc.float32_gap(case), hc.stored_gaps()[cid]
    assert got["zero"] == stored["zero"] == []
    assert sorted(got["blocks"]) == sorted(stored["blocks"])
    for key, floor, cap in (("loss", 1e-6, 2.5e-4), ("z", 1.5e-6, 2.5e-4)):      # a quarter of compare_losses' 1e-3
        assert got[key] <= 1.5 * max(stored[key], floor), (key, got[key], stored[key])
        assert got[key] <= cap
    lost = [k for k, v in stored["blocks"].items() if hc.bar_of(v) is None]
    assert len(lost) <= hc.MAX_LOST * max(1, len(stored["blocks"]))
    for name, gap in got["blocks"].items():
        assert gap <= 1.5 * max(stored["blocks"][name], hc.GAP_FLOOR), (name, gap, stored["blocks"][name])
        bar = hc.bar_of(stored["blocks"][name])
        assert bar is not None and gap <= hc.QUARTER * bar, (name, gap, bar)


def test_stored_gaps_set_the_plain_bar_everywhere():
    """What the cases file states: every block's gap is at most 3.1e-5 (d / d md, k1l1), so every bar is 2e-3 and no case
    loses a block; loss gap at most 1.0e-6 of the largest loss, z gap at most 1.3e-6 absolute."""
    s = hc.stored_gaps()
    worst = max((v, cid, k) for cid in hc.GRAD_IDS for k, v in s[cid]["blocks"].items())
    assert worst[0] <= 3.2e-5 and worst[1] == "k1l1" and worst[2].startswith("md"), worst
    assert all(hc.bar_of(v) == hc.BAR for cid in hc.GRAD_IDS for v in s[cid]["blocks"].values())
    assert s["refdefault"]["blocks"] == {}
    assert max(s[cid]["loss"] for cid in hc.IDS) <= 1.05e-6 and max(s[cid]["z"] for cid in hc.IDS) <= 1.35e-6
