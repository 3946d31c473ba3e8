"""The d = 1600 gradients (cmcd_lgcp.hip: lgcp_grad, lgcp_uha_grad, the deferred contractions) at the pass, tile and width edges
of tests/lgcp_grad_cases.py: every leaf against autograd through the float64 restatement in the blocks different code writes,
each block under the bar of DESIGN.md section 2 ("Gradients at d = 1600"); shards, n_total, repeats, a call at another size in
between, and the batch order."""
import json

import numpy as np
import pytest
import torch

import lgcp_grad_cases as lc
from cmcd_amd import mcdboundingmachine as mcdbm
from helpers import compare_losses

pytestmark = pytest.mark.gpu


def _dev(seeds):
    return torch.from_numpy(np.ascontiguousarray(seeds)).cuda()


def _np64(t):
    return t.double().cpu().numpy()


@pytest.mark.parametrize("param_set", lc.PARAM_SETS)
@pytest.mark.parametrize("cid", lc.IDS)
def test_lgcp_gradient_cases_match_autograd(hip_lib, monkeypatch, cid, param_set):
    """Every case on both parameter sets: losses and z through helpers.compare_losses and equal in bits to the forward-only call
    on the same seeds (both run the 32-row sequence at these n), no non-finite reference loss, every block of every leaf under
    its bar, exactly zero where the reference is.

    What this test found (round 18): d / d eps of the VarGrad call, [var-n52-dense] 5.7e-3 of its maximum 143.5 against the bar
    2e-3 and 5.3e-2 on [var-n17-sparse].  lgcp_adj_elem redrew the forward kernel's noise while the backward kernel's residual came
    from the stored float32 states, so the rounding of each stored state times 2 df / (4 eps^2) did not cancel.  With both from the
    stored states: 1.8e-4 and 2.2e-3, at most 7e-4 on the eight others."""
    case = lc.case_by_id(cid)
    _, mode, n, K, form, _ = case
    monkeypatch.setattr(mcdbm, "KERNEL_VARIANT", form)
    b = lc.build(case, param_set)
    seeds = _dev(lc.seeds_of(case))
    grad, (losses, z) = lc.call(b, seeds)
    l_fwd, z_fwd, _ = lc.forward(b, seeds)
    torch.cuda.synchronize()
    _, l_ref, z_ref, g_ref = lc.reference(case, param_set)
    assert np.isfinite(l_ref).all() and bool(torch.isfinite(grad).all())
    g = _np64(grad)
    rep, bad = lc.compare_blocks(case, param_set, b["unflatten"], g, g_ref, tag=cid)
    l, zz = _np64(losses), _np64(z)
    obs = dict(case=cid, params=param_set, loss=lc.worst_particle(l, l_ref), z=lc.z_error(zz, z_ref),
               worst=sorted(((v, k) for k, v in rep.items()), reverse=True)[:4],
               fwd_bits=bool(torch.equal(losses, l_fwd) and torch.equal(z, z_fwd)))
    print("OBS", json.dumps(obs))
    compare_losses(l, l_ref, zz, z_ref, tag=cid, K=K)
    assert obs["fwd_bits"], "losses / z of the gradient call differ from the forward-only call's"
    assert not bad, bad
    if mode == lc.UHA:          # the 2nd-order family's own bars on the losses and z (lc.uha_loss_bars)
        loss_bar, z_bar = lc.uha_loss_bars()
        assert obs["loss"] <= loss_bar and obs["z"] <= z_bar, (cid, obs["loss"], loss_bar, obs["z"], z_bar)


def _at_form(monkeypatch, b, seeds, form):
    monkeypatch.setattr(mcdbm, "KERNEL_VARIANT", form)
    grad, (losses, z) = lc.call(b, seeds)
    return grad.clone(), losses.clone(), z.clone()


@pytest.mark.parametrize("cid", ["uha-w3332-5", "uha-w3332-37"])
def test_the_library_takes_the_split_k_sequence_beyond_3328_inputs(hip_lib, monkeypatch, cid):
    """IN = 3332 > 32 kNskChunks: lgcp_uha_nsk_ok is false, so form 0 is the sequence form 3 pins — gradient, losses and z in
    the same bits."""
    case = lc.case_by_id(cid)
    assert case[4] == 0 and lc.route_of(case) == ("split-k", "recompute")
    b = lc.build(case, "dense")
    seeds = _dev(lc.seeds_of(case))
    own = _at_form(monkeypatch, b, seeds, 0)
    pinned = _at_form(monkeypatch, b, seeds, 3)
    assert bool(torch.isfinite(own[0]).all()) and float(own[0].abs().max()) > 0
    for a, r, what in zip(own, pinned, ("gradient", "losses", "z")):
        assert torch.equal(a, r), (cid, what, float((a - r).abs().max()))


@pytest.mark.parametrize("cid", ["uha-w3328-20", "uha-rc-n20"])
def test_the_two_2nd_order_sequences_agree(hip_lib, monkeypatch, cid):
    """Widths the no-split-K form takes (3328: the last one; 3220): form 0 (no-split-K forward, sweep on kept activations) against
    form 3 (split-K forward, recompute sweep) on the same seeds.  They differ in summation order only: every block within
    SHARD_TOL of its maximum, losses and z within the rounding tolerances test_lgcp_wide_batch_path_matches_oracle gives two
    forms of one path."""
    case = lc.case_by_id(cid)
    dim, emb, K, n = lc.D, case[5].get("emb_dim", 20), case[3], case[2]
    assert lc.uha_route(dim, emb, K, n, 0) == ("nsk", "kept") and lc.uha_route(dim, emb, K, n, 3) == ("split-k", "recompute")
    b = lc.build(case, "dense")
    seeds = _dev(lc.seeds_of(case))
    g0, l0, z0 = _at_form(monkeypatch, b, seeds, 0)
    g3, l3, z3 = _at_form(monkeypatch, b, seeds, 3)
    errs = lc.block_errors(b["unflatten"], _np64(g3), _np64(g0))
    worst = max((e / s, k) for k, (e, s) in errs.items() if s > 0)
    print("OBS", json.dumps(dict(forms=cid, worst=worst, loss=float((l3 - l0).abs().max()), z=float((z3 - z0).abs().max()),
                                 same_bits=bool(torch.equal(g0, g3)))))
    assert float(g0.abs().max()) > 0
    bad = {k: (e, s) for k, (e, s) in errs.items() if not e <= lc.SHARD_TOL * s}
    assert not bad, bad
    np.testing.assert_allclose(l3.cpu().numpy(), l0.cpu().numpy(), rtol=2e-5, atol=2e-3)
    np.testing.assert_allclose(z3.cpu().numpy(), z0.cpu().numpy(), rtol=1e-5, atol=1e-5)


SHARDS = [("n33", 21), ("n52", 32), ("ulasn-n33", 21), ("ulasn-n52", 32), ("uha-n33", 21), ("uha-n52", 32), ("var-n33", 21),
          ("var-n52", 32), ("uha-rc-n33", 21)]


@pytest.mark.parametrize("cid,cut", SHARDS)
def test_shards_add_up(hip_lib, monkeypatch, cid, cut):
    """Multi-GPU contract: two particle shards called with n_total = the whole batch (VarGrad: and the whole batch's statistics
    as stats_total) sum to the single call's gradient, per block within 1e-4 of the block's maximum.

    What this test found (round 18): [var-n52-32], block `eps`, 3.8e-4, and 3.2e-5 .. 3.6e-5 on the same block of n33 / n52 — every
    particle keeps its pass size and row, so that was the grouping of lgcp_adj_reduce_kernel's float32 sums, multiplied by
    1 / (4 eps^2) = 62 500.  With the sums in float64 the worst block of any pair is 5.6e-6."""
    case = lc.case_by_id(cid)
    monkeypatch.setattr(mcdbm, "KERNEL_VARIANT", case[4])
    b = lc.build(case, "dense")
    seeds = _dev(lc.seeds_of(case))
    n = seeds.numel()
    kw = dict(n_total=n)
    if case[1] == lc.VAR:
        kw["stats_total"] = lc.forward(b, seeds)[2].clone()
    g_all, _ = lc.call(b, seeds)
    g_all = _np64(g_all)
    g_a, _ = lc.call(b, seeds[:cut].contiguous(), **kw)
    g_a = _np64(g_a)
    g_b, _ = lc.call(b, seeds[cut:].contiguous(), **kw)
    errs = lc.block_errors(b["unflatten"], g_a + _np64(g_b), g_all)
    worst = max((e / s, k) for k, (e, s) in errs.items() if s > 0)
    print("OBS", json.dumps(dict(shards=cid, worst=worst)))
    assert float(np.abs(g_all).max()) > 0
    bad = {k: (e, s) for k, (e, s) in errs.items() if not e <= lc.SHARD_TOL * s}
    assert not bad, bad


@pytest.mark.parametrize("cid", ["n33", "ulasn-n17", "ula-n20", "uha-n17", "uha-rc-n20"])
def test_n_total_scales_the_gradient(hip_lib, monkeypatch, cid):
    """n_total = 2 n halves every entry bit for bit; losses and z do not depend on it."""
    case = lc.case_by_id(cid)
    monkeypatch.setattr(mcdbm, "KERNEL_VARIANT", case[4])
    b = lc.build(case, "dense")
    seeds = _dev(lc.seeds_of(case))
    n = seeds.numel()
    g_all, (l_all, z_all) = lc.call(b, seeds)
    g_all, l_all, z_all = g_all.clone(), l_all.clone(), z_all.clone()
    g_one, _ = lc.call(b, seeds, n_total=n)
    assert torch.equal(g_one, g_all)
    g_half, (l_h, z_h) = lc.call(b, seeds, n_total=2 * n)
    assert float(g_all.abs().max()) > 0
    assert torch.equal(g_half * 2, g_all)
    assert torch.equal(l_h, l_all) and torch.equal(z_h, z_all)


@pytest.mark.parametrize("cid", ["n20", "n52", "n65", "rc-n33", "var-n21", "uha-rc-n33"])
def test_repeated_calls_are_bitwise_identical(hip_lib, monkeypatch, cid):
    """Six calls, with an unrelated launch in between: gradient, losses and z in the same bits.  The two-stream recompute and the
    split-K tickets are where a missing ordering would show (uha-rc-n33: the 2nd-order sequence's slab tickets and the counters
    its two passes share)."""
    case = lc.case_by_id(cid)
    monkeypatch.setattr(mcdbm, "KERNEL_VARIANT", case[4])
    b = lc.build(case, "dense")
    seeds = _dev(lc.seeds_of(case))
    first = None
    noise = torch.randn(1 << 20, device="cuda")
    for rep in range(6):
        if rep % 2 == 1:
            noise = noise * 1.0001
        grad, (losses, z) = lc.call(b, seeds)
        got = (grad.clone(), losses.clone(), z.clone())
        if first is None:
            first = got
            assert bool(torch.isfinite(got[0]).all()) and bool(torch.isfinite(got[1]).all())
        else:
            for a, r, what in zip(got, first, ("gradient", "losses", "z")):
                assert torch.equal(a, r), (rep, what, float((a - r).abs().max()))


@pytest.mark.parametrize("cid", ["n52", "var-n52", "uha-n52", "uha-rc-n65"])
def test_a_call_at_another_size_in_between_changes_nothing(hip_lib, monkeypatch, cid):
    """Gradient at n = 52 (65 on uha-rc-n65, at its form), then at n = 5, then at the first size again on the same workspace: the
    third equals the first in bits (stale packed-operand padding, stale kept rows or stale slabs of the 5-row pass would show)."""
    case = lc.case_by_id(cid)
    monkeypatch.setattr(mcdbm, "KERNEL_VARIANT", case[4])
    b = lc.build(case, "dense")
    seeds = _dev(lc.seeds_of(case))
    g1, (l1, z1) = lc.call(b, seeds)
    g1, l1, z1 = g1.clone(), l1.clone(), z1.clone()
    g5, _ = lc.call(b, seeds[:5].contiguous())
    assert bool(torch.isfinite(g5).all()) and not torch.equal(g5, g1)
    g3, (l3, z3) = lc.call(b, seeds)
    assert torch.equal(g3, g1) and torch.equal(l3, l1) and torch.equal(z3, z1)


@pytest.mark.parametrize("cid", ["n33", "var-n33", "uha-rc-n33"])
def test_batch_order(hip_lib, monkeypatch, cid):
    """n = 33 reversed: the same gradient, per block within the shard tolerance; the losses and z permuted in bits — a particle's
    loss does not depend on its row / pass, except for passes of 17 .. 20 particles, where rows 16 .. 19 share a workgroup with
    rows 0 .. 15 and a particle that moves across row 16 changes in the last bits of every product (none at n = 33).
    uha-rc-n33, the 2nd-order split-K sequence: in bits too.  lgcp_gemm_kernel gives every output row the same K-slices, the same
    quarter per wave and the same 32x32x2 MFMA chain whatever its row index, the padding rows it contracts beside are zeros of
    other rows' outputs, the slabs are summed in slab order per element, and lgcp_uha_init / mid / close_kernel<4> run one
    workgroup per particle: nothing in a particle's arithmetic knows its row or pass.

    What this test found (round 18): [var-n33], block `eps`, 4.7e-4 against 1e-4, from the same float32 sums as in
    test_shards_add_up."""
    case = lc.case_by_id(cid)
    monkeypatch.setattr(mcdbm, "KERNEL_VARIANT", case[4])
    b = lc.build(case, "dense")
    seeds = _dev(lc.seeds_of(case))
    n = seeds.numel()
    assert not any(16 < m <= 20 for m in lc.passes_of(n))
    kw = dict(stats_total=lc.forward(b, seeds)[2].clone()) if case[1] == lc.VAR else {}
    g0, (l0, z0) = lc.call(b, seeds, **kw)
    g0, l0, z0 = _np64(g0), l0.clone(), z0.clone()
    g1, (l1, z1) = lc.call(b, seeds.flip(0).contiguous(), **kw)
    assert torch.equal(l1, l0.flip(0)) and torch.equal(z1, z0.flip(0))
    errs = lc.block_errors(b["unflatten"], _np64(g1), g0)
    bad = {k: (e, s) for k, (e, s) in errs.items() if not e <= lc.SHARD_TOL * s}
    assert not bad, bad
