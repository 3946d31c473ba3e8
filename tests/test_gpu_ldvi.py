"""LDVI on the GPU — cmcd_amd.ldvi over cmcd_ldvi_bound_grad (cmcd_amd/csrc/cmcd_ldvi.hip) — against the float64 restatement of
tests/ldvi_restatement.py, which tests/test_ldvi_oracle.py pins on the CPU, on identical seeds and parameters (tests/ldvi_cases.py:
the dense parameter set; what each shape is there for is asserted on the CPU).

Bars, the project's: losses, z and the five statistics through tests/helpers.compare_losses / check_stats; every gradient leaf cut
where different kernels write it (the sn leaves from the item kernel's slabs and rows and the embedding tail, vd and gamma from the
sweep, eps and mgridref_y through the schedule tail), each held to max(2e-3 of its own maximum, 4 x the recorded float32 gap of the
restatement on that block) — tests/golden/ldvi_gaps.json, kept current by the CPU test."""
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
    for case_id in (lc.SHARED, "funnel"):
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
