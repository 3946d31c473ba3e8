"""Pins tests/reverse_hais_restatement.py (the float64 yardstick of cmcd_bound_reverse_hais and cmcd_amd.reverse_hais) without a
device: evaluated on a forward path of UHA it is the forward restatement's functional (w(path) = -loss of
tests/hais_restatement.py, and the inverted leap-frogs walk back to the path's z_0 and initial momentum); its free-running
deviates are reverse_uha_restatement.reverse_deviates' (the forward chain's without its first draw); and at L = 3 the chain that
treats every inner kick as a half-kick is far from it on the case tests/test_gpu_reverse_hais.py uses.

The path identity is held to the bar of tests/test_reverse_uha_oracle.py, 1e-9 (rtol and atol); md is non-zero and eta = 0.6 in every
case (hais_restatement.make_params).  Measured here, max |w + loss| over the six cases: 2.2e-14 (gmm), 2.9e-14 (funnel), 1.8e-13 (many_gmm) —
the funnel's neck needs no looser bar at K = 8."""
import functools

import numpy as np
import pytest

import hais_restatement as hr
import reverse_hais_restatement as rh
from oracle import prng
from oracle import targets as otg
from reverse_uha_restatement import reverse_deviates

# (dim, eps, q's sigma, scale of q's mean): tests/test_gpu_hais.py's
TARGETS = {"gmm": (2, 0.05, 2.0, 1.0), "funnel": (10, 0.05, 1.0, 0.5), "many_gmm": (2, 0.1, 15.0, 5.0)}
ORACLE_TARGET = {"gmm": otg.Gmm, "funnel": lambda: otg.Funnel(10), "many_gmm": otg.ManyGmm}
PARITY_BAR = 1e-3      # helpers.compare_losses: the worst particle of a K <= 32 chain


@functools.lru_cache(maxsize=None)
def built(name, K, L, device="cpu", eta=0.6):
    dim, eps, sigma, mean_scale = TARGETS[name]
    flat, un, fixed = hr.make_params(dim, K, L, eps, seed=K + 10 * L, device=device, mean_scale=mean_scale, sigma=sigma, eta=eta)
    return flat, un, fixed, hr.params_numpy(un, flat)


@pytest.mark.parametrize("name", ["gmm", "funnel", "many_gmm"])
@pytest.mark.parametrize("L", [1, 3])
def test_on_a_forward_path_it_is_the_forward_restatements_functional(name, L):
    K, n = 8, 24
    _, _, (dim, _, _), p = built(name, K, L)
    assert np.abs(p["md"]).max() > 0.05 and float(p["eta"]) == pytest.approx(0.6)
    tgt = ORACLE_TARGET[name]()
    seeds = np.arange(1, n + 1, dtype=np.int32)
    loss, zK = hr.forward(seeds, p, dim, K, L, name)
    assert np.isfinite(loss).all()
    path = rh.forward_path(seeds, p, dim, K, L, tgt)
    assert len(path) == K + 1
    np.testing.assert_allclose(path[K][0], zK, rtol=1e-9, atol=1e-9)      # the path is the forward restatement's
    w, z0, rho0 = rh.reverse_chain_hais(seeds, path[K][0], p, dim, K, L, tgt, path=path)
    print(name, L, "max |w + loss|", np.abs(w + loss).max(), "max |z0 - path z0|", np.abs(z0 - path[0][0]).max())
    np.testing.assert_allclose(w, -loss, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(z0, path[0][0], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(rho0, path[0][2], rtol=1e-9, atol=1e-9)      # s normal(R): the forward chain's initial momentum


def test_the_free_running_deviates_are_reverse_deviates():
    seeds = np.array([1, 2, 77, 123456, 2 ** 31 - 1], np.int32)
    for dim, K in ((2, 8), (10, 5)):
        rho_k, xi = reverse_deviates(seeds, dim, K)
        e0, n0, noise = prng.particle_noise_uha(seeds, dim, K)
        assert np.array_equal(rho_k, n0) and all(np.array_equal(xi[:, r], noise[:, r]) for r in range(K))
        assert not any(np.array_equal(e0, d) for d in [rho_k] + [xi[:, r] for r in range(K)])      # none is the forward chain's first draw
    # the chain consumes exactly these: K = 1, L = 1 at eps -> 0 leaves rho_0 = eta s normal(R) + sqrt(1 - eta^2) s xi_0
    _, _, (dim, K, L), p = built("gmm", 1, 1)
    p = dict(p, eps=np.asarray(0.0))
    x = np.zeros((len(seeds), 2))
    _, z0, rho0 = rh.reverse_chain_hais(seeds, x, p, dim, K, L, otg.Gmm())
    rho_k, xi = reverse_deviates(seeds, 2, 1)
    s, eta = np.exp(p["md"]), float(p["eta"])
    assert np.array_equal(z0, x)
    np.testing.assert_allclose(rho0, eta * s * rho_k + np.sqrt(1.0 - eta * eta) * s * xi[:, 0], rtol=1e-14, atol=1e-14)


def test_at_three_leapfrog_steps_the_inner_kicks_are_full_kicks():
    """The GPU test's case: gmm, n = 37, K = 8, L = 3."""
    n, K, L = 37, 8, 3
    _, _, (dim, _, _), p = built("gmm", K, L)
    from cmcd_amd.model_handler import exact_target_draws, load_model
    x = exact_target_draws("gmm", load_model("gmm", None)[2], 5, n, dim)
    seeds = np.arange(1, n + 1, dtype=np.int32)
    w, _, _ = rh.reverse_chain_hais(seeds, x, p, dim, K, L, otg.Gmm())
    w_bad, _, _ = rh.reverse_chain_hais_inner_half_kicks(seeds, x, p, dim, K, L, otg.Gmm())
    gap = (np.abs(w_bad - w) / np.maximum(1.0, np.abs(w))).max()
    print("gap", gap)
    assert gap > 100 * PARITY_BAR
    # ... and at L = 1 there is no inner kick: the two are the same chain
    _, _, _, p1 = built("gmm", K, 1)
    assert np.array_equal(rh.reverse_chain_hais(seeds, x, p1, dim, K, 1, otg.Gmm())[0],
                          rh.reverse_chain_hais_inner_half_kicks(seeds, x, p1, dim, K, 1, otg.Gmm())[0])


def test_a_non_finite_row_of_x_gives_plus_infinity_and_leaves_the_others_alone():
    _, _, (dim, K, L), p = built("gmm", 8, 1)
    seeds = np.arange(1, 6, dtype=np.int32)
    x = np.random.default_rng(1).normal(size=(5, dim))
    clean = rh.reverse_chain_hais(seeds, x, p, dim, K, L, otg.Gmm())
    x[1, 0], x[3, 1] = np.nan, -np.inf
    w, z0, rho0 = rh.reverse_chain_hais(seeds, x, p, dim, K, L, otg.Gmm())
    assert w[1] == np.inf and w[3] == np.inf and not np.isnan(w).any()
    for got, ref in zip((w, z0, rho0), clean):
        assert np.array_equal(got[[0, 2, 4]], ref[[0, 2, 4]])
