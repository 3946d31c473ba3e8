"""tests/lgcp_grad_cases.py from the restatement alone (no GPU): each case is what its header says, the float32 gap behind every
bar is the stored one, the block cuts tile every leaf once, the float32 switch of the lgcp log-density left the float64 results
alone, and two independent statements of the same gradient agree (the sharding contract tests/test_gpu_lgcp_grad.py uses)."""
import numpy as np
import pytest
import torch

import lgcp_grad_cases as lc
from helpers import lgcp_counts_fixture
from oracle import cmcd_oracle_torch as ot


def test_cases_are_what_their_header_says():
    assert len(set(lc.IDS)) == len(lc.IDS) and set(lc.PASSES) == set(lc.IDS) == set(lc.stored_gaps())
    for cid, mode, n, K, form, over in lc.CASES:
        assert 1 <= K <= 3 and 1 <= n <= 129 and form in (0, 3), cid
        assert lc.PASSES[cid] == lc.passes_of(n) and sum(lc.PASSES[cid]) == n, cid
        assert over.get("eps_schedule") != "linear" or K > 1, cid
    kind = lambda cid: [lc.gemm_of(m) for m in lc.PASSES[cid]]
    assert kind("n16") == ["nsk"] and kind("n17") == ["merged"] and kind("n20") == ["merged"] and kind("n21") == ["split-k"]
    assert kind("n33") == ["split-k", "nsk"] and kind("n52") == ["split-k", "merged"] and len(kind("n65")) == 3
    assert len(kind("n129")) == 5 > 4                                             # one more pass than the forward has lanes
    for fam in ("var-", "ulasn-", "uha-"):                                        # the merged instance in every family
        assert any(kind(c) [-1] == "merged" for c in lc.IDS if c.startswith(fam)), fam
    assert {lc.case_by_id(c)[3] for c in ("n21", "n129", "rc-n21", "uha-n52")} == {1}
    widths = {c: lc.D + lc.case_by_id(c)[5].get("emb_dim", 20) for c in lc.IDS}
    assert widths["w1612-21"] == 1612 and 1612 % 16 and 1612 % 128 and -(-1612 // 16) == 101
    assert widths["w1670-5"] > 1664 >= widths["n20"]                               # 16 kNskChunks: lgcp_nsk_ok
    assert {lc.case_by_id(c)[4] for c in lc.IDS if c.startswith("rc-")} == {3}
    assert {lc.case_by_id(c)[4] for c in lc.IDS if c.startswith("uha-rc-")} == {3}
    assert {c: lc.case_by_id(c)[4] for c in lc.IDS if c.startswith("uha-w")} == dict.fromkeys(
        ("uha-w3332-5", "uha-w3332-37", "uha-w3328-20", "uha-w3212-37", "uha-w3204-20"), 0)
    assert {lc.case_by_id(c)[3] for c in ("uha-rc-n21",)} == {1} and lc.case_by_id("uha-rc-n33")[3] == 3
    uw = {c: 2 * lc.D + lc.case_by_id(c)[5].get("emb_dim", 20) for c in lc.UHA_IDS}
    assert all(c.startswith("uha-") for c in lc.UHA_IDS) and len(lc.UHA_IDS) == 16
    assert all(uw[c] == int(c.split("-")[1][1:]) for c in lc.UHA_IDS if c.startswith("uha-w"))
    assert -(-3332 // 64) == 53 and 3332 % 64 == 4                                  # cbIN with a 4-column last block
    assert 3328 == 32 * lc.NSK_CHUNKS and 3328 % 16 == 0                             # exactly 2 x 104 chunks, nothing ragged
    assert -(-3212 // 16) == 201 and 3212 % 16 == 12 and 3204 % 16 == 4              # tIN ragged
    assert kind("uha-w3328-20") == kind("uha-w3204-20") == ["merged"] and kind("uha-w3212-37") == ["split-k", "nsk"]


def test_2nd_order_cases_take_the_forward_and_the_sweep_they_say():
    """lgcp_uha_nsk_ok and the keep budget of lgcp_uha_grad_ws restated (lc.uha_route): which forward form and which sweep every
    uha-* case runs — the split-K forward and the recompute sweep by the pin (form 3) and by the library's own choice (IN = 3332),
    the no-split-K forward with the sweep on kept activations everywhere else, up to the last width it takes."""
    assert set(lc.UHA_ROUTES) == set(lc.UHA_IDS)
    for cid in lc.UHA_IDS:
        case = lc.case_by_id(cid)
        assert lc.route_of(case) == lc.UHA_ROUTES[cid], (cid, lc.route_of(case))
        pinned, own = case[4] == 3, 2 * lc.D + case[5].get("emb_dim", 20) > 32 * lc.NSK_CHUNKS
        assert lc.UHA_ROUTES[cid] == (("split-k", "recompute") if pinned or own else ("nsk", "kept")), cid
    assert not any(lc.case_by_id(c)[4] == 3 for c in ("uha-w3332-5", "uha-w3332-37"))             # the library's own choice
    # the boundary of lgcp_uha_nsk_ok, IN = 3328 | 3332 (emb_dim is a multiple of 4 here), and d itself
    assert lc.uha_nsk_ok(lc.D, 128, 0) and not lc.uha_nsk_ok(lc.D, 132, 0) and not lc.uha_nsk_ok(lc.D, 128, 3)
    assert lc.uha_nsk_ok(1664, 0, 0) and not lc.uha_nsk_ok(1680, 0, 0) and not lc.uha_nsk_ok(1608, 20, 0)
    # the same rules as tests/capture_cases.py restates them for its own table
    import capture_cases as cc
    for cid in lc.UHA_IDS:
        assert cc.lgcp_facts(lc.case_by_id(cid))["kept"] == (lc.UHA_ROUTES[cid][1] == "kept"), cid
    # no case comes near the budget: the (nsk, recompute) route is the one no case takes
    assert ("nsk", "recompute") not in lc.UHA_ROUTES.values()
    assert max(lc.uha_keep_floats(lc.D, c[5].get("emb_dim", 20), c[3], c[2]) for c in lc.CASES if c[1] == lc.UHA) < lc.KEEP_FLOATS // 50


def test_keep_budget_at_width_3220():
    """The production route no case can afford: at width 3220 the kept tables are 17 680 K n + 1600 n floats (lgcp_uha_grad_ws:
    R (2 IN + D) + (K + 1) n D with R = 2 K n), and past 2^28 of them the library runs the no-split-K forward followed by the
    recompute sweep.  The first K n at which that happens."""
    dim, emb = lc.D, 20
    IN = 2 * dim + emb
    assert IN == 3220 and 2 * (2 * IN + dim) + dim == 17680
    assert lc.uha_keep_floats(dim, emb, 7, 11) == 17680 * 77 + 1600 * 11
    on = lambda K, n: lc.uha_route(dim, emb, K, n, 0) == ("nsk", "kept")
    off = lambda K, n: lc.uha_route(dim, emb, K, n, 0) == ("nsk", "recompute")
    k1 = lc.UHA_KEEP_OFF_KN["k1"]                     # K = 1: K n = n, 19 280 n floats
    assert on(1, k1 - 1) and off(1, k1) and k1 == (1 << 28) // 19280 + 1
    anyk = lc.UHA_KEEP_OFF_KN["any"]                  # n = 1, the least the n D term can be: off from here on for every (K, n)
    assert on(anyk - 1, 1) and off(anyk, 1) and 17680 * anyk > (1 << 28) - 1600
    assert all(off(K, -(-anyk // K)) for K in (1, 2, 3, 8, 32, 128, 256))
    assert all(on(K, (k1 - 1) // K) for K in (1, 2, 3, 8, 32, 128, 256))                # ... and on for every (K, n) below k1
    n128 = lc.UHA_KEEP_OFF_N_AT_K128                  # the configuration's K
    assert on(128, n128 - 1) and off(128, n128) and n128 == 119 and k1 <= 128 * n128 and 128 * (n128 - 1) < anyk
    # form 3 and the widths beyond 3328 never keep
    assert lc.uha_route(dim, emb, 1, 1, 3) == ("split-k", "recompute") == lc.uha_route(dim, 132, 1, 1, 0)


def test_2nd_order_loss_bars_come_from_the_stored_gaps():
    """lc.uha_loss_bars: FACTOR x the largest stored gap of any uha-* case, on the worst particle and on z; both within a quarter
    of compare_losses' 1e-3."""
    loss_bar, z_bar = lc.uha_loss_bars()
    gaps = [lc.stored_gaps()[cid][ps] for cid in lc.UHA_IDS for ps in lc.PARAM_SETS]
    assert len(gaps) == 32
    assert loss_bar == lc.FACTOR * max(g["loss"] for g in gaps) and z_bar == lc.FACTOR * max(g["z"] for g in gaps)
    assert 0 < loss_bar <= lc.QUARTER * 1e-3 and 0 < z_bar <= lc.QUARTER * 1e-3
    print("2nd-order bars: loss %.3e z %.3e" % (loss_bar, z_bar))


@pytest.mark.parametrize("param_set", lc.PARAM_SETS)
@pytest.mark.parametrize("cid", lc.IDS)
def test_float32_gap_is_the_stored_one(cid, param_set):
    """Re-measures `float32_gap` and holds the golden record to it: a listed block within 1.5 x of its stored gap (both ways where
    the gap sets the bar), an unlisted one below 1.5 x LISTED, every bar at least FACTOR x the gap, the losses and z within a
    quarter of compare_losses' 1e-3, the named tiny / zero blocks the same, and no more than MAX_LOST of the blocks lost."""
    case = lc.case_by_id(cid)
    gap, stored = lc.float32_gap(case, param_set), lc.stored_gap(case, param_set)
    worst = sorted(gap["blocks"].items(), key=lambda kv: -kv[1])[:3]
    print(cid, param_set, "loss %.2e z %.2e" % (gap["loss"], gap["z"]), "worst blocks", [(k, "%.1e" % v) for k, v in worst])
    assert gap["tiny"] == stored["tiny"] and gap["zero"] == stored["zero"]
    assert gap["loss"] <= 1.5 * stored["loss"] and gap["z"] <= 1.5 * stored["z"]
    assert stored["loss"] <= lc.QUARTER * 1e-3 and stored["z"] <= lc.QUARTER * 1e-3
    bar, lost = lc.bars(case, param_set)
    assert set(stored["blocks"]) <= set(gap["blocks"])
    for name, g in gap["blocks"].items():
        s = stored["blocks"].get(name)
        if s is None:
            assert g <= 1.5 * lc.LISTED, (name, g)
            assert bar(name) == lc.BAR
            continue
        assert s > lc.LISTED and g <= 1.5 * s, (name, g, s)
        if s > lc.QUARTER * lc.BAR:                 # the gap sets the bar (or loses the block): not overstated either
            assert s <= 1.5 * g, (name, g, s)
        if name not in lost:
            assert s <= lc.QUARTER * bar(name) and (bar(name) == lc.BAR or bar(name) == lc.FACTOR * s), (name, s, bar(name))
    nblocks = len(gap["blocks"]) + len(gap["zero"])
    assert len(lost) <= lc.MAX_LOST * nblocks, (lost, nblocks)


@pytest.mark.parametrize("cid", lc.IDS)
def test_block_cuts_tile_each_leaf_exactly_once(cid):
    b = lc.build(lc.case_by_id(cid), "sparse", device="cpu")
    numel = b["params_flat"].numel()
    bl = lc.blocks(b["unflatten"], np.arange(numel, dtype=np.float64))
    names = [name for name, _, _ in bl]
    assert len(set(names)) == len(names)
    hit = np.zeros(numel, np.int64)
    for _, a, covers in bl:
        assert a.size > 0
        if covers:
            np.add.at(hit, a.reshape(-1).astype(np.int64), 1)
    assert hit.min() == 1 == hit.max()
    whole = {name: a for name, a, covers in bl if not covers}
    assert set(whole) == {"vd.mean", "vd.logdiag"} and all(a.size == lc.D for a in whole.values())
    if not cid.startswith("ula-"):
        emb = b["unflatten"].shape("sn", "emb")[1]
        assert emb == lc.case_by_id(cid)[5].get("emb_dim", 20)
        rows = 2 * lc.D if cid.startswith("uha") else lc.D
        by = dict((n, a) for n, a, _ in bl)
        assert by["W1.emb.cols"].shape == (emb, rows)
        if cid.startswith("uha"):        # the state rows of the 2nd-order mode: z rows [:D], rho rows [D:2D]
            assert "W1.state.cols" not in by and "W1.state.lastcols" not in by
            assert by["W1.z.cols"].shape == by["W1.rho.cols"].shape == (lc.D, rows)
            assert by["W1.z.lastcols"].shape == by["W1.rho.lastcols"].shape == (lc.D, emb)
            assert by["W1.z.cols"][0, 0] + lc.D * (rows + emb) == by["W1.rho.cols"][0, 0]
        else:
            assert by["W1.state.lastcols"].shape == (rows, emb) and "W1.z.cols" not in by
        assert by["W2.lastcols"].shape == (rows + emb, emb) and by["W3.last64"].shape == (rows + emb, 64)
        assert by["b3.last64"].shape == (64,) and by["vd.mean[1536:1600]"].shape == (64,)


def test_float64_results_did_not_change_with_the_float32_switch():
    """make_logp_lgcp casts its two constant tensors to the dtype of z; at float64 every result keeps its bits (against the
    log-density as it stood before the cast, written out here)."""
    from oracle.targets import Lgcp
    t = Lgcp(lgcp_counts_fixture())
    kinv, counts = torch.tensor(t.kinv), torch.tensor(t.counts)

    def before(z):
        r = z - t.mu0
        return -0.5 * ((r @ kinv) * r).sum(-1) + (z * counts - t.a * torch.exp(z)).sum(-1) + t.lognorm
    for cid in ("n16", "var-n17"):
        case = lc.case_by_id(cid)
        new = lc.reference(case, "dense")
        old = lc.run_restatement(case, "dense", logp=before)
        assert new[0] == old[0]
        for a, r in zip(new[1:], old[1:]):
            assert a.dtype == np.float64 and np.array_equal(a, r)
    with pytest.raises(RuntimeError):               # what the switch is for: the old form cannot run at float32
        lc.run_restatement(lc.case_by_id("n1"), "dense", dtype=torch.float32, logp=before)


@pytest.mark.parametrize("cid", ["n33", "ulasn-n33", "uha-n33"])
def test_gradient_of_the_mean_is_the_share_weighted_sum_of_its_shards(cid):
    """bound_and_grad over 33 seeds == 21 / 33 of the call on seeds[:21] + 12 / 33 of the call on seeds[21:]: what n_total asks
    of the device (each shard scaled by 1 / n_total instead of 1 / its own n)."""
    case = lc.case_by_id(cid)
    seeds = lc.seeds_of(case)
    _, l, z, g = lc.reference(case, "dense")
    _, la, za, ga = lc.run_restatement(case, "dense", seeds=seeds[:21])
    _, lb, zb, gb = lc.run_restatement(case, "dense", seeds=seeds[21:])
    assert np.array_equal(np.concatenate([la, lb]), l) and np.array_equal(np.concatenate([za, zb]), z)
    s = (21.0 * ga + 12.0 * gb) / 33.0
    assert np.abs(g).max() > 0
    assert np.abs(s - g).max() <= 1e-12 * np.abs(g).max()


def test_vargrad_is_autograd_of_the_variance_of_the_concatenated_shard_losses():
    """MCD_CAIS_var_sn: the gradient of var(losses) over 33 seeds == autograd of var(cat(losses of seeds[:21], losses of
    seeds[21:])): the weights 2 (l_p - mean) / n_total need the merged statistics (stats_total), not a shard's own."""
    case = lc.case_by_id("var-n33")
    b = lc.build(case, "dense", device="cpu")
    dim, K, mode, spec = b["params_fixed"]
    seeds = lc.seeds_of(case)
    p = ot.to_torch(lc.oracle_params_of(b))
    logp = ot.make_logp_lgcp(lgcp_counts_fixture())
    parts = [ot.losses(s, p, dim, K, mode, spec.arch, logp, b["cfg"]["eps_schedule"], b["cfg"]["grad_clipping"])[0]
             for s in (seeds[:21], seeds[21:])]
    value = torch.cat(parts).var(unbiased=False)
    un = b["unflatten"]
    _, _, _, g = lc.reference(case, "dense")
    checked = 0
    for path, leaf in ((("vd", "mean"), p["vd"]["mean"]), (("vd", "logdiag"), p["vd"]["logdiag"]), (("eps",), p["eps"]),
                       (("sn", "nn", 2, 1), p["sn"]["b3"]), (("sn", "emb"), p["sn"]["emb"]),
                       (("sn", "nn", 0, 0), p["sn"]["W1"])):
        (got,) = torch.autograd.grad(value, leaf, retain_graph=True)
        off = un.offset(*path)
        want = g[off:off + got.numel()]
        assert np.abs(want).max() > 0
        assert np.abs(got.numpy().reshape(-1) - want).max() <= 1e-10 * np.abs(want).max(), path
        checked += 1
    assert checked == 6
