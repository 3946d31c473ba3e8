"""Pins tests/reverse_ldvi_restatement.py (the float64 yardstick of cmcd_bound_reverse_ldvi and cmcd_amd.reverse_ldvi) without a
device: evaluated on a forward path of the mode it is the forward restatement's functional (w(path) = -loss of
tests/ldvi_restatement.py, and the inverted leap-frogs walk back to the path's (z_0, rho_0)); its free-running deviates are
reverse_uha_restatement.reverse_deviates' (the forward chain's without its first draw); and the two deliberately wrong chains are far
from it on the case tests/test_gpu_reverse_ldvi.py uses.

The path identity is held to the bar of tests/test_reverse_uha_oracle.py, 1e-9 (rtol and atol); measured here, max |w + loss|: gmm K = 8
4e-15, funnel K = 4 2e-14, many_gmm K = 8 2.4e-11, network-free 7e-15 — the funnel's neck needs no looser bar at K = 4."""
import numpy as np
import pytest

import ldvi_cases as lc
import ldvi_restatement as lr
import reverse_ldvi_restatement as rl
from cmcd_amd import synthetic
from helpers import oracle_target
from oracle import prng
from reverse_uha_restatement import reverse_deviates

# (id, ldvi_cases case): LDVI gmm K = 8, funnel K = 4, many_gmm K = 8 and the network-free mode
CASES = [("gmm-k8", "gmm-n33"), ("funnel-k4", "funnel"), ("many_gmm-k8", "many-n33"), ("nonet", "nonet")]
PARITY_BAR = 1e-3      # helpers.compare_losses: the worst particle of a K <= 32 chain


def pieces(case_id):
    b = lc.build(case_id)
    dim, K, mode, _ = b["params_fixed"]
    return b, rl.params_numpy(b["unflatten"], b["params_flat"]), dim, K, mode == "MCD_U_a-lp-sn", oracle_target(b["cfg"])


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_on_a_forward_path_it_is_the_forward_restatements_functional(case):
    tag, case_id = case
    b, p, dim, K, use_sn, tgt = pieces(case_id)
    assert K == {"gmm-k8": 8, "funnel-k4": 4, "many_gmm-k8": 8, "nonet": 8}[tag]
    seeds = lc.seeds_of(case_id)[:24]
    p_lr, _, model = lc.params_of(case_id)
    loss, zK = lr.forward(seeds, p_lr, dim, K, model, use_sn=use_sn)
    path = rl.forward_path(seeds, p, dim, K, tgt)
    assert len(path) == K + 1
    np.testing.assert_allclose(path[K][0], zK, rtol=1e-9, atol=1e-9)      # the path is the forward restatement's
    fin = np.isfinite(loss)
    assert fin.sum() >= 17
    w, z0, rho0 = rl.reverse_chain_ldvi(seeds, path[K][0], p, dim, K, tgt, use_sn=use_sn, path=path)
    print(tag, "max |w + loss|", np.abs(w[fin] + loss[fin]).max(), "max |z0 - path z0|", np.abs(z0[fin] - path[0][0][fin]).max(),
          "max |rho0 - path rho0|", np.abs(rho0[fin] - path[0][1][fin]).max())
    np.testing.assert_allclose(w[fin], -loss[fin], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(z0[fin], path[0][0][fin], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(rho0[fin], path[0][1][fin], rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("dim,K", [(2, 8), (10, 5)])
def test_the_free_running_deviates_are_reverse_deviates(dim, K):
    """reverse_deviates is the forward chain's noise without its first draw, none of its arrays IS that first draw, and the
    free-running chain consumes exactly reverse_deviates(seeds, dim, K) (seen through a wrapper around the function it calls)."""
    seeds = np.array([1, 2, 77, 123456, 2 ** 31 - 1], np.int32)
    rho_k, xi = reverse_deviates(seeds, dim, K)
    e0, rho0_fwd, noise = prng.particle_noise_uha(seeds, dim, K)
    assert np.array_equal(rho_k, rho0_fwd) and all(np.array_equal(xi[:, r], noise[:, r]) for r in range(K))
    assert not any(np.array_equal(e0, d) for d in [rho_k] + [xi[:, r] for r in range(K)])      # none is the forward chain's first draw
    # the chain itself: K = 1 on gmm, where rho_0 - m_b = sigma xi_0 and rho_K enters w through log N(rho_K; 0, I) alone
    if dim == 2:
        b, p, _, _, _, tgt = pieces("gmm-k1")
        x = np.zeros((len(seeds), 2))
        got = {}
        orig = rl.reverse_deviates
        try:
            rl.reverse_deviates = lambda s, d, k: got.setdefault("dev", orig(s, d, k))
            rl.reverse_chain_ldvi(seeds, x, p, 2, 1, tgt)
        finally:
            rl.reverse_deviates = orig
        rk1, xi1 = reverse_deviates(seeds, 2, 1)
        assert np.array_equal(got["dev"][0], rk1) and np.array_equal(got["dev"][1], xi1)


def gpu_wrong_chain_case(device="cpu"):
    """The case tests/test_gpu_reverse_ldvi.py holds the device apart from the wrong chains on: gmm, K = 4, eps = 0.05, the
    embedding table scaled by 40 so that the bridge index counts."""
    b = lc.build("gmm-n33", device=device)
    b2 = synthetic.build("gmm_n300_k8", device=device, dense=True, boundmode="MCD_CAIS_UHA_sn", nbridges=4, init_eps=0.05)
    flat = b2["params_flat"].clone()
    off, shape = b2["unflatten"].layout[(0, "sn", "emb")]
    flat[off:off + int(np.prod(shape))] *= 40.0
    dim, K, _, spec = b2["params_fixed"]
    return dict(b2, params_flat=flat, params_fixed=(dim, K, b["params_fixed"][2], spec))


def wrong_chain_inputs(b, n=33):
    from cmcd_amd.model_handler import exact_target_draws, load_model
    sampler = load_model(b["cfg"]["model"], None)[2]
    return synthetic.parity_seeds(n), exact_target_draws(b["cfg"]["model"], sampler, 5, n, b["params_fixed"][0])


def test_the_wrong_chains_are_far_from_the_right_one():
    b = gpu_wrong_chain_case()
    seeds, x = wrong_chain_inputs(b)
    w, _, _ = rl.run_restatement(b, seeds, x)
    for chain in (rl.reverse_chain_ldvi_backward_at_next_index, rl.reverse_chain_ldvi_forward_mean_with_network):
        w_bad, _, _ = rl.run_restatement(b, seeds, x, chain=chain)
        gap = (np.abs(w_bad - w) / np.maximum(1.0, np.abs(w))).max()
        print(chain.__name__, "gap", gap)
        assert gap > 100 * PARITY_BAR


def test_a_non_finite_row_of_x_gives_plus_infinity_and_leaves_the_others_alone():
    b, p, dim, K, use_sn, tgt = pieces("gmm-k1")
    seeds = synthetic.parity_seeds(5)
    x = np.random.default_rng(1).normal(size=(5, dim))
    clean = rl.reverse_chain_ldvi(seeds, x, p, dim, K, tgt)
    x[1, 0], x[3, 1] = np.nan, -np.inf
    w, z0, rho0 = rl.reverse_chain_ldvi(seeds, x, p, dim, K, tgt)
    assert w[1] == np.inf and w[3] == np.inf and not np.isnan(w).any()
    for got, ref in zip((w, z0, rho0), clean):
        assert np.array_equal(got[[0, 2, 4]], ref[[0, 2, 4]])
