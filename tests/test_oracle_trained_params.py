"""What tests/trained_cases.py says about its cases, asserted from the oracles alone (no HIP code runs here): the trained
snapshots are trained, the corner cases sit on the faces of the projection box, the seed lists are what the guard band leaves, and
the float32 gaps that set the bars of tests/test_gpu_trained.py are what the stored tables say."""
import numpy as np
import pytest
import torch

import gated_cases as gc
import trained_cases as tc
from cmcd_amd import synthetic

CASES, IDS = tc.CASES, tc.IDS
TRAINED = [c for c in CASES if tc.is_trained(c)]
CORNERS = [c for c in CASES if not tc.is_trained(c)]
_GRAD = {}


def grad_pair(case):
    """(float64, float32) runs of the gradient oracle on the case as its gradient comparisons run it, once per case."""
    if case[0] not in _GRAD:
        b = tc.build_case(case, grad=True)
        _GRAD[case[0]] = (b, tc.grad_oracle(b, case[3]), tc.grad_oracle(b, case[3], dtype=torch.float32))
    return _GRAD[case[0]]


def test_the_case_list_covers_the_issue_and_stays_small():
    assert len(set(IDS)) == len(IDS) and set(tc.N0) == set(IDS) == set(tc.LOSS_GAP32)
    assert set(tc.GRAD_GAP32) <= set(IDS) and set(tc.DROPPED) <= set(IDS)
    rows = tc.TRAINED_ROWS
    assert {r["boundmode"] for r in rows.values()} == {"MCD_CAIS_sn", "MCD_CAIS_var_sn", "MCD_CAIS_UHA_sn", "MCD_ULA_sn",
                                                       "MCD_ULA", "UHA"}
    assert {r["model"] for r in rows.values()} == {"gmm", "funnel", "many_gmm"}
    assert {r["nn_arch"] for r in rows.values()} == {"geffner", "dds"}
    assert rows["many-dds"]["nbridges"] == 64 and rows["many-dds"]["grad_clipping"]       # 33 grid nodes under 64 bridges
    for cid, r in rows.items():
        assert r["emb_dim"] <= 48 and r["nbridges"] <= 64, cid
    for c in CASES:
        assert tc.N0[c[0]] <= 64 and tc.bridges_of(c) <= 64, c[0]
    lo = [c for c in CORNERS if c[2].get("init_eps") == tc.EPS_LO]
    hi = [c for c in CORNERS if c[2].get("init_eps") == tc.EPS_HI]
    assert {c[1] for c in lo} >= {"gmm_n300_k8", "funnel_n300_k64", "many_gmm_n2000_k256_dds", "many_gmm_var_n16000_k256"}
    assert {c[1] for c in hi} == {"funnel_n300_k64", "many_gmm_n2000_k256_dds"}            # not gmm: its chain is unstable there
    glo = [c for c in CORNERS if c[2].get("init_gamma") == tc.GAMMA_LO]
    assert all(c[4] == "MCD_CAIS_UHA_sn" for c in glo)
    assert {(c[1], c[2]["init_eps"]) for c in glo} >= {(m, e) for m in ("gmm_n300_k8", "funnel_n300_k64") for e in (0.2, tc.EPS_LO)}
    grid = [c for c in CORNERS if c[2].get("grid") == "floored"]
    assert sorted(tc.bridges_of(c) for c in grid).count(40) >= 2 and any(tc.bridges_of(c) == 8 and c[4] != "UHA" for c in grid)
    assert any(c[4] == "UHA" for c in grid)
    assert any(c[2].get("init_eps") == tc.EPS_LO and c[2].get("init_gamma") == tc.GAMMA_LO and c[2].get("grid") for c in CORNERS)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_seeds_are_the_survivors_of_the_guard_band(case):
    n0 = tc.N0[case[0]]
    assert tc.select_seeds(case) == tuple(case[3])
    assert n0 - len(case[3]) <= n0 // 8, "more than one seed in eight dropped: change the case"


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_losses_are_finite_or_infinite_alike_and_the_float32_gap_is_the_stored_one(case):
    """No NaN and no -inf; float32 and float64 agree on which particles are +inf (forward_gap32 asserts it); the recomputed
    gap may not exceed the stored one by more than a factor 1.5, so that a changed fixture cannot silently loosen a bar."""
    b = tc.build_case(case)
    l64, _ = tc.forward_oracle(b, case[3])
    assert not np.isnan(l64).any() and not (l64 == -np.inf).any() and np.isfinite(l64).sum() >= len(l64) // 2
    gap = tc.forward_gap32(case)
    print(case[0], {k: "%.2e" % v for k, v in gap.items()})
    for m in tc.LOSS_METRICS:
        assert gap[m] <= 1.5 * tc.LOSS_GAP32[case[0]][m], (m, gap[m], tc.LOSS_GAP32[case[0]][m])
    # a loosened bar never loosens the p99 / mean / ln Z bounds beyond the worst-particle one, and stays a bound
    bars = tc.loss_bars(case[0], tc.bridges_of(case))
    assert all(np.isfinite(v) and v <= 0.2 for v in bars.values())


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_gradient_float32_gap_is_the_stored_one_and_below_the_cap(case):
    """Per leaf max |g32 - g64| / max |g64| of the autograd oracle: listed leaves within 1.5 x the stored value, every other
    leaf within 1.5 x GRAD_LISTED; no stored value above GRAD_CAP (the corner is moved inwards instead: grad_eps); the float64
    gradient is finite, also where losses are +inf."""
    b, (l64, _, g64), (l32, _, g32) = grad_pair(case)
    assert bool(torch.isfinite(g64).all()) and float(g64.abs().max()) > 0
    if case[4] != "MCD_CAIS_var_sn":
        assert np.array_equal(np.isinf(l32), np.isinf(l64))
    gap = tc.leaf_errors(b["unflatten"], g32, g64)
    stored = tc.GRAD_GAP32.get(case[0], {})
    print(case[0], {k: "%.2e" % v for k, v in gap.items()})
    assert set(stored) <= set(gap), set(stored) - set(gap)
    for leaf, v in gap.items():
        assert v <= 1.5 * stored.get(leaf, tc.GRAD_LISTED), (leaf, v, stored.get(leaf))
    assert all(tc.GRAD_LISTED < v <= tc.GRAD_CAP for v in stored.values()), stored
    assert tc.QUARTER * gc.BAR > 1.5 * tc.GRAD_LISTED                  # an unlisted leaf is on the standard bar by right
    # the float32 restatement itself passes the whole-vector check of test_gpu_grad._compare
    cos = float((g32 * g64).sum() / (g32.norm() * g64.norm()))
    assert cos > 1 - 1e-5, cos


@pytest.mark.parametrize("case", CORNERS, ids=[c[0] for c in CORNERS])
def test_corner_case_sits_on_its_face(case):
    cid, config, over, seeds, mode = case
    b = tc.build_case(case)
    m = np.asarray(tc.leaf_value(b, "mgridref_y"), np.float64)
    if "init_eps" in over and over["init_eps"] in (tc.EPS_LO, tc.EPS_HI):
        assert float(tc.leaf_value(b, "eps")) == float(np.float32(over["init_eps"]))
    if "init_gamma" in over:
        assert over["init_gamma"] == tc.GAMMA_LO and float(tc.leaf_value(b, "gamma")) == float(np.float32(tc.GAMMA_LO))
    if "grad_eps" in over:      # the gradient runs of the case: the same parameters but for eps
        bg = tc.build_case(case, grad=True)
        assert float(tc.leaf_value(bg, "eps")) == float(np.float32(over["grad_eps"])) and over["init_eps"] == tc.EPS_LO
        diff = (bg["params_flat"] != b["params_flat"]).nonzero().reshape(-1).tolist()
        assert diff == [next(v for p, v in b["unflatten"].layout.items() if p[1:] == ("eps",))[0]]
    if "out_scale" in over:     # the clamp's neighbourhood: outputs a kernel clamping at 1e3 would cut, none the true one cuts
        trace = {}
        tc.grad_oracle(b, seeds, trace=trace)
        out = np.abs(gc._stack(trace, "out"))
        print(cid, "share of dds outputs in (1e3, 1e4): %.2f, beyond: %.2f" % (((out > 1e3) & (out < 1e4)).mean(), (out >= 1e4).mean()))
        assert ((out > 1.5e3) & (out < 0.9e4)).mean() > 0.1 and not (out >= 1e4).any()
    if over.get("grid") == "floored":
        K = tc.bridges_of(case)
        assert float(m.min()) == float(np.float32(tc.GRID_FLOOR)) and (m == m.min()).sum() >= len(m) // 3
        # bridge i lies in cell j of the grid (ot.betas_from_grid); the cell's width is m[j - 1] / sum(m)
        pos = np.arange(1, K + 1, dtype=np.float64) / (K + 1) * len(m)
        j = np.clip(np.floor(pos).astype(np.int64) + 1, 1, len(m))
        width = m[j - 1] / m.sum()
        narrow = width < 1e-2 / len(m)
        print(cid, "bridges in near-empty cells:", int(narrow.sum()), "of", K, "off the nodes:", int((pos != np.floor(pos)).sum()))
        assert narrow.any()
        if K == 40 or mode == "UHA":
            assert (narrow & (pos != np.floor(pos))).any(), "no bridge INSIDE a near-empty cell"
        else:
            assert (pos == np.floor(pos)).all()                     # on the nodes
        betas = tc.ot.betas_from_grid(torch.tensor(m), K).numpy()
        assert (np.diff(betas) >= 0).all()
        if K == 40:        # 40 bridges over 33 cells: two of them share a near-empty cell, so their betas all but coincide
            assert (np.diff(betas) < 1e-2 / len(m)).any()


@pytest.mark.parametrize("case", TRAINED, ids=[c[0] for c in TRAINED])
def test_trained_snapshot_differs_from_the_start_in_every_trainable_leaf(case):
    """... and in no other: a fixture swapped for the initial parameters fails here."""
    row = tc.TRAINED_ROWS[case[0]]
    b, b0 = tc.build_case(case), tc.initial_build(row)
    assert b["unflatten"].layout == b0["unflatten"].layout
    trainable = tc.trainable_of(row)
    moved = {}
    for path, (off, shape) in b["unflatten"].layout.items():
        n = max(1, int(np.prod(shape)))
        moved[path[1:]] = float((b["params_flat"][off:off + n] - b0["params_flat"][off:off + n]).abs().max())
    print(case[0], {"/".join(map(str, k)): "%.2e" % v for k, v in moved.items()})
    for path, d in moved.items():
        # eta (every MCD mode) and gamma (the overdamped ones) are trainable leaves that no loss depends on
        dead = (path[0] == "eta" and row["boundmode"] != "UHA") or (path[0] == "gamma" and row["boundmode"] != "MCD_CAIS_UHA_sn")
        if (path[0] in trainable or path[0] == "sn") and not dead:
            assert d > 1e-3, f"{path}: a trainable leaf at its initial value"
        else:
            assert d == 0.0, f"{path}: a leaf outside the trainable set moved"
    if "sn" in {p[0] for p in moved} and row["nn_arch"] == "geffner":
        assert abs(float(tc.leaf_value(b, "sn", "factor_sn"))) > 0.01      # the network has grown from its zero start
    m = tc.leaf_value(b, "mgridref_y")
    assert float(m.min()) >= 1e-3 and float(m.max() / m.min()) > 1.5       # a beta grid far from uniform, inside the box
    flags, _ = tc.load_fixture(case[0])
    assert flags == row


def test_the_torch_oracle_at_float32_is_the_same_arithmetic():
    """dtype=torch.float32 changes the precision and nothing else: float64 by default (same bits as before the argument
    existed is pinned by tests/test_oracle_grad.py), float32 within single-precision distance of it."""
    case = tc.case_by_id("grid-gmm")
    b, (l64, z64, g64), (l32, z32, g32) = grad_pair(case)
    l_np, z_np = tc.forward_oracle(b, case[3])
    np.testing.assert_allclose(l64, l_np, rtol=1e-9, atol=1e-9)
    assert 0 < np.abs(l32 - l64).max() < 1e-4 and 0 < float((g32 - g64).abs().max()) < 1e-4 * float(g64.abs().max())
    p = tc.oracle_params(b)
    assert all(t.dtype == torch.float32 for t in (tc.ot.to_torch(p, dtype=torch.float32)["eps"], tc.ot.to_torch(p, dtype=torch.float32)["sn"]["W1"]))
    assert tc.ot.to_torch(p)["eps"].dtype == torch.float64
