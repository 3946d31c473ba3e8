"""LDVI on the GPU — cmcd_amd.ldvi over cmcd_ldvi_bound_grad (cmcd_amd/csrc/cmcd_ldvi.hip) — against the float64 restatement of
tests/ldvi_restatement.py, which tests/test_ldvi_oracle.py pins on the CPU, on identical seeds and parameters (tests/ldvi_cases.py:
the dense parameter set; what each shape is there for is asserted on the CPU).

Bars, the project's: losses, z and the five statistics through tests/helpers.compare_losses / check_stats; every gradient leaf cut
where different kernels write it (the sn leaves from the item kernel's slabs and rows and the embedding tail, vd and gamma from the
sweep, eps and mgridref_y through the schedule tail), each held to max(2e-3 of its own maximum, 4 x the recorded float32 gap of the
restatement on that block) — tests/golden/ldvi_gaps.json, kept current by the CPU test.

Beside the parity cases: what the call keeps between calls and across streams (repeats, a call at another size in between, a side
stream, a captured call replayed twice), shards on either side of the item kernel's 512-workgroup cap, a reversed batch, and the
statistics with 4 and 8 waves per forward workgroup."""
import functools
import math
import types

import numpy as np
import pytest
import torch

import ldvi_cases as lc
import ldvi_restatement as lr
from cmcd_amd import ldvi, opt
from helpers import check_stats, compare_losses

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def built(case_id):
    return lc.build(case_id, device="cuda")


def dev(seeds):
    return torch.from_numpy(np.asarray(seeds, np.int32)).cuda()


def args_of(case_id):
    b = built(case_id)
    return b["params_flat"], b["unflatten"], b["params_fixed"], b["target"]


@functools.lru_cache(maxsize=None)
def device_gradient(case_id):
    """One gradient call per case, shared (read-only) by the tests that look at it."""
    grad, (losses, z) = ldvi.grad_and_loss(dev(lc.seeds_of(case_id)), *args_of(case_id))
    torch.cuda.synchronize()
    return grad, losses, z


@pytest.mark.parametrize("case_id", sorted(lc.CASES))
def test_bound_and_gradient_match_the_restatement(hip_lib, case_id):
    l_ref, z_ref, g_ref = lc.reference(case_id)
    seeds = lc.seeds_of(case_id)
    K = built(case_id)["params_fixed"][1]
    losses, z, stats = ldvi.bound_forward(dev(seeds), *args_of(case_id))
    torch.cuda.synchronize()
    # the +inf set matches exactly (compare_losses asserts it), the finite particles and their z under the project's bar
    rep = compare_losses(losses.cpu().numpy(), l_ref, z.cpu().numpy(), z_ref, tag=case_id, K=K)
    print(case_id, rep, check_stats(stats, losses, tag=case_id))
    if case_id == "many-floor":
        assert int(torch.isinf(losses).sum()) >= 4 and bool((losses[torch.isinf(losses)] > 0).all())
    grad, l_g, z_g = device_gradient(case_id)
    # the forward-only call returns the gradient call's losses and z bit for bit
    assert torch.equal(l_g, losses) and torch.equal(z_g, z)
    assert bool(torch.isfinite(grad).all())
    lc.compare_blocks(case_id, built(case_id)["unflatten"], grad, g_ref)


def test_compute_bound_is_the_statistics_mean(hip_lib):
    seeds = dev(lc.seeds_of(lc.SHARED))
    losses, z, stats = ldvi.bound_forward(seeds, *args_of(lc.SHARED))
    mean, (l2, z2) = ldvi.compute_bound(seeds, *args_of(lc.SHARED))
    assert torch.equal(l2, losses) and torch.equal(z2, z)
    assert float(mean) == float((stats[1] / losses.numel()).to(torch.float32))
    assert abs(float(mean) - float(losses.double().mean())) <= 1e-5 * max(1.0, abs(float(mean)))


def test_one_bridge_pins_the_draws(hip_lib):
    """K = 1: z_1 - z_0 = eps (rho' - eps/2 gU(z_0)) with z_0 the restatement's own draw: the deviates of q, of the initial
    momentum and of the refresh are the key chain's, in that order."""
    p, (dim, K, _, _), _ = lc.params_of("gmm-k1")
    seeds = lc.seeds_of("gmm-k1")
    e0, _, _ = lr.noise(seeds, dim, K)
    z0 = (np.exp(p["vd"]["logdiag"]) * e0.numpy() + p["vd"]["mean"])
    _, z_ref, _ = lc.reference("gmm-k1")
    _, _, z = device_gradient("gmm-k1")
    step, step_ref = z.double().cpu().numpy() - z0, z_ref - z0
    assert np.abs(step_ref).max() > 1e-3
    assert np.abs(step - step_ref).max() <= 1e-3 * np.abs(step_ref).max() + 4 * np.finfo(np.float32).eps * np.abs(z0).max()


def test_repeated_gradient_calls_are_bitwise_identical(hip_lib):
    """Per-item and per-tile slots summed in a fixed order, no float atomics."""
    for case_id in (lc.SHARED, "funnel", "gmm-slabs", "gmm-w44"):
        first = device_gradient(case_id)
        noise = torch.randn(1 << 18, device="cuda")
        for rep in range(3):
            noise = noise * 1.0001   # an unrelated launch in between
            grad, (losses, z) = ldvi.grad_and_loss(dev(lc.seeds_of(case_id)), *args_of(case_id))
            assert torch.equal(grad, first[0]) and torch.equal(losses, first[1]) and torch.equal(z, first[2]), (case_id, rep)


def test_gradient_shards_add_up(hip_lib):
    """Shards called with the size of the whole batch sum to the single call's gradient (33 = 20 + 13: other tiles, other sums)."""
    seeds = dev(lc.seeds_of(lc.SHARED))
    n = seeds.numel()
    g_all, _, _ = device_gradient(lc.SHARED)
    g_a, _ = ldvi.grad_and_loss(seeds[:20], *args_of(lc.SHARED), n_total=n)
    g_b, _ = ldvi.grad_and_loss(seeds[20:], *args_of(lc.SHARED), n_total=n)
    un = built(lc.SHARED)["unflatten"]
    for name, (e, s) in lr.block_errors(un, (g_a + g_b).cpu(), g_all.cpu()).items():
        assert e <= 1e-4 * s, (name, e, s)      # float32 sums in another order: a few ulps of the largest term


def _assert_shards_add_up(case_id, cut):
    seeds = dev(lc.seeds_of(case_id))
    n = seeds.numel()
    g_all, l_all, z_all = device_gradient(case_id)
    g_a, (l_a, z_a) = ldvi.grad_and_loss(seeds[:cut].contiguous(), *args_of(case_id), n_total=n)
    g_b, (l_b, z_b) = ldvi.grad_and_loss(seeds[cut:].contiguous(), *args_of(case_id), n_total=n)
    # cut on a tile boundary or not, a particle's own chain does not depend on its batch
    assert torch.equal(torch.cat([l_a, l_b]), l_all) and torch.equal(torch.cat([z_a, z_b]), z_all)
    worst = 0.0
    for name, (e, s) in lr.block_errors(built(case_id)["unflatten"], (g_a + g_b).cpu(), g_all.cpu()).items():
        assert e <= 1e-4 * s, (case_id, name, e, s)      # the bar of test_gradient_shards_add_up
        worst = max(worst, e / s if s > 0 else 0.0)
    print(case_id, "shards %d + %d: worst block %.1e of its maximum" % (cut, n - cut, worst))


def test_shards_across_the_slab_cap(hip_lib):
    """gmm-slabs as 128 + 80: the shards hold 8 x 40 = 320 and 5 x 40 = 200 items, one per workgroup, the whole batch 520 on 512
    workgroups, eight of which walk two; funnel-slabs as 65 + 64: 5 x 64 = 320 and 4 x 64 = 256 items against 576."""
    K = {c: built(c)["params_fixed"][1] for c in ("gmm-slabs", "funnel-slabs")}
    assert K["gmm-slabs"] * 8 == 320 and K["gmm-slabs"] * 5 == 200 and K["gmm-slabs"] * 13 == 520 > 512   # 512: kLdviMaxSlabs
    assert K["funnel-slabs"] * 5 == 320 and K["funnel-slabs"] * 4 == 256 and K["funnel-slabs"] * 9 == 576 > 512
    _assert_shards_add_up("gmm-slabs", 128)
    _assert_shards_add_up("funnel-slabs", 65)


def test_a_call_at_another_size_in_between_changes_nothing(hip_lib):
    """The workspace keeps the slabs, rows and kept states of the previous call: gmm-slabs (520 items, a walk), gmm-k40 (the same
    parameters, 80 items, no walk), gmm-slabs again."""
    assert torch.equal(built("gmm-slabs")["params_flat"], built("gmm-k40")["params_flat"])
    first = device_gradient("gmm-slabs")
    alone = device_gradient("gmm-k40")
    g1, (l1, z1) = ldvi.grad_and_loss(dev(lc.seeds_of("gmm-slabs")), *args_of("gmm-slabs"))
    g2, (l2, z2) = ldvi.grad_and_loss(dev(lc.seeds_of("gmm-k40")), *args_of("gmm-k40"))
    g3, (l3, z3) = ldvi.grad_and_loss(dev(lc.seeds_of("gmm-slabs")), *args_of("gmm-slabs"))
    torch.cuda.synchronize()
    for got, want in (((g1, l1, z1), first), ((g2, l2, z2), alone), ((g3, l3, z3), first)):
        assert all(torch.equal(a, b) for a, b in zip(got, want))
    assert torch.equal(g3, g1) and torch.equal(l3, l1) and torch.equal(z3, z1)


def test_batch_order(hip_lib):
    """gmm-slabs-k33 with its seeds reversed: every particle sits in another lane, tile and slab (the one-particle tile now holds
    seed 1); losses and z follow their seeds bit for bit, the gradient is the same sum in another order."""
    case_id = "gmm-slabs-k33"
    g_all, l_all, z_all = device_gradient(case_id)
    seeds = dev(lc.seeds_of(case_id)[::-1].copy())
    grad, (losses, z) = ldvi.grad_and_loss(seeds, *args_of(case_id))
    torch.cuda.synchronize()
    assert torch.equal(losses.flip(0), l_all) and torch.equal(z.flip(0), z_all)
    for name, (e, s) in lr.block_errors(built(case_id)["unflatten"], grad.cpu(), g_all.cpu()).items():
        assert e <= 1e-4 * s, (name, e, s)      # float32 sums in another order: a few ulps of the largest term


def _slabs_call(with_grad, seeds):
    if with_grad:
        g, (l, z) = ldvi.grad_and_loss(seeds, *args_of("gmm-slabs"))
        return g, l, z
    return ldvi.bound_forward(seeds, *args_of("gmm-slabs"))


def _assert_same_bits(got, want, with_grad, tag):
    bad = []
    for name, a, b in zip(("grad", "losses", "z") if with_grad else ("losses", "z", "stats"), got, want):
        if not torch.equal(a, b):
            off = torch.nonzero((a != b).flatten()).flatten()
            bad.append("%s: %d of %d entries differ, first at %s: %s against %s" % (
                name, off.numel(), a.numel(), off[:8].tolist(), a.flatten()[off[:4]].tolist(), b.flatten()[off[:4]].tolist()))
    assert not bad, (tag, bad)


@pytest.mark.parametrize("with_grad", [False, True])
def test_non_default_stream(hip_lib, with_grad):
    seeds = dev(lc.seeds_of("gmm-slabs"))
    eager = [t.clone() for t in _slabs_call(with_grad, seeds)]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out = _slabs_call(with_grad, seeds)
    side.synchronize()
    _assert_same_bits(out, eager, with_grad, "side stream")
    if with_grad:
        _assert_same_bits(out, device_gradient("gmm-slabs"), with_grad, "side stream against the shared call")


@pytest.mark.parametrize("with_grad", [False, True])
def test_captured_call_replays_the_eager_bits(hip_lib, with_grad):
    """One linear stream: every launch of the call on the capture stream, in order.  The second replay follows the zeroing of the
    outputs without a host synchronisation: with two memset nodes in the graph the gradient call returned garbage there in d eps,
    the last embedding row, b1 and W1[2 d:] (ldvi_zero_kernel replaced them)."""
    static = dev(lc.seeds_of("gmm-slabs"))
    eager = [t.clone() for t in _slabs_call(with_grad, static)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _slabs_call(with_grad, static)                              # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        captured = _slabs_call(with_grad, static)
    for rep in range(2):
        for t in captured:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        _assert_same_bits(captured, eager, with_grad, "replay %d" % rep)


@pytest.mark.parametrize("case_id", ["gmm-nw4", "gmm-nw8"])
def test_statistics_beyond_one_wave_per_workgroup(hip_lib, case_id):
    """4 and 8 waves per forward workgroup: the per-tile records are written by sibling waves, the last workgroup has one live
    wave.  The five statistics against the returned losses, and compute_bound's mean against their float64 mean."""
    seeds = dev(lc.seeds_of(case_id))
    tiles = (seeds.numel() + 15) // 16
    assert (tiles > 1024, tiles > 8192) == {"gmm-nw4": (True, False), "gmm-nw8": (True, True)}[case_id]
    losses, z, stats = ldvi.bound_forward(seeds, *args_of(case_id))
    print(case_id, check_stats(stats, losses, tag=case_id))
    mean, (l2, z2) = ldvi.compute_bound(seeds, *args_of(case_id))
    assert torch.equal(l2, losses) and torch.equal(z2, z)
    want = float(losses.double().mean())
    assert abs(float(mean) - want) <= 1e-6 * abs(want), (float(mean), want)


def test_trainable_subset(hip_lib):
    """trainable = (eps, gamma): the other leaves sit in params_notrain and come back exactly zero; the two kept ones carry the
    full call's values (same kernels, same sums)."""
    b = built(lc.SHARED)
    dim, K, mode, spec = b["params_fixed"]
    train, notrain = b["unflatten"](b["params_flat"].cpu())
    allp = {**train, **notrain}
    flat, un, fixed = ldvi.initialize(dim, vdparams=allp["vd"], nbridges=K, eps=float(allp["eps"]), gamma=float(allp["gamma"]),
                                      eta=float(allp["eta"]), mgridref_y=allp["mgridref_y"], trainable=("eps", "gamma"),
                                      emb_dim=spec.emb_dim, mode=mode, nn_arch="geffner", device="cpu")
    sub_train, _ = un(flat)
    # the network's leaves stay in params_train (the reference puts sn there whatever `trainable` says): copy the case's values
    for (w, bias), (w0, b0) in zip(sub_train["sn"]["nn"], allp["sn"]["nn"]):
        w.copy_(w0)
        bias.copy_(b0)
    sub_train["sn"]["emb"].copy_(allp["sn"]["emb"])
    sub_train["sn"]["factor_sn"].copy_(allp["sn"]["factor_sn"])
    flat = flat.cuda()
    grad, (losses, _) = ldvi.grad_and_loss(dev(lc.seeds_of(lc.SHARED)), flat, un, fixed, b["target"])
    g_all, l_all, _ = device_gradient(lc.SHARED)
    assert torch.equal(losses, l_all)
    full = b["unflatten"]
    for name in ("eps", "gamma"):
        assert float(grad[un.offset(name)]) == float(g_all[full.offset(name)]) != 0.0
    for name in (("vd", "mean"), ("vd", "logdiag"), ("mgridref_y",), ("eta",)):
        off, shape = un.offset(*name), un.shape(*name)
        assert float(grad[off:off + max(1, int(np.prod(shape)))].abs().max()) == 0.0, name
    assert float(g_all[full.offset("vd", "mean")].abs()) > 0


def test_training_lowers_the_loss_and_reproduces(hip_lib):
    """20 steps of opt.run on gmm, n = 32, K = 4 from the reference's start: the mean loss on fresh seeds drops, and the run
    reproduces bit for bit from its seed."""
    trainable = ("eta", "gamma", "eps", "vd", "mgridref_y")
    flat, un, fixed = ldvi.initialize(2, nbridges=4, eps=0.05, gamma=4.0, trainable=trainable, emb_dim=20, mode="MCD_U_a-lp-sn",
                                      nn_arch="geffner", device="cuda")
    tgt = built(lc.SHARED)["target"]
    fresh = dev(np.arange(2_000_001, 2_000_001 + 2048))
    before, _ = ldvi.compute_bound(fresh, flat, un, fixed, tgt)
    info = types.SimpleNamespace(N=32)
    runs = []
    for _ in range(2):
        losses, trained, _ = opt.run(info, 0.01, 20, flat.clone(), un, fixed, tgt, ldvi.grad_and_loss, trainable, 7)
        runs.append(trained.clone())
    assert torch.equal(runs[0], runs[1])
    after, _ = ldvi.compute_bound(fresh, runs[0], un, fixed, tgt)
    print("LDVI gmm K = 4: mean loss", float(before), "->", float(after))
    assert math.isfinite(float(after)) and float(after) < float(before)
    sn_before, sn_after = un(flat)[0]["sn"], un(runs[0])[0]["sn"]
    assert not torch.equal(sn_before["factor_sn"], sn_after["factor_sn"])     # the network trains (factor_sn starts at 0)


@pytest.mark.parametrize("boundmode", ldvi.MODES)
def test_driver_routes_the_ldvi_modes(hip_lib, capsys, boundmode):
    """python -m cmcd_amd.main --config.boundmode MCD_U_a-lp[-sn]: trains and evaluates on one GPU with the reference's
    trainable tuple (main.py:137-146)."""
    from cmcd_amd import main as cli
    argv = ["--config.model", "gmm", "--config.boundmode", boundmode, "--config.N", "16", "--config.nbridges", "4",
            "--config.mfvi_iters", "20", "--config.iters", "20", "--config.n_samples", "32", "--config.n_input_dist_seeds", "3",
            "--config.init_eps", "0.01", "--config.lr", "0.001", "--noconfig.compute_w2"]
    elbo, ln_z = cli.main(cli.parse_flags(argv, cli.get_config()))
    out = capsys.readouterr().out
    assert math.isfinite(elbo) and math.isfinite(ln_z) and elbo <= ln_z
    assert "Params being trained : ('eta', 'gamma', 'eps', 'vd', 'mgridref_y')" in out
