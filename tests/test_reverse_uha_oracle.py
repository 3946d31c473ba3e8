"""Pins tests/reverse_uha_restatement.py (the float64 yardstick of cmcd_bound_reverse_uha and cmcd_amd.reverse_uha) without a
device: evaluated on a forward path of the mode it is the forward oracle's functional (w(path) = -loss of
oracle.compute_log_elbo_batch_uha, and the inverted leap-frogs walk back to the path's z_0); one bridge agrees with the listing
written out by hand; and its deviates are the forward chain's (oracle.prng.particle_noise_uha) without the first draw.

The many_gmm cases run at init_eps = 0.05: the configurations' own step sizes give gamma eps > 1 (tests/test_gpu_smc_uha.py)."""
import numpy as np
import pytest

from cmcd_amd import synthetic
from helpers import oracle_target
from oracle import cmcd_oracle as orc
from oracle import prng
import reverse_uha_restatement as rr

MODE = "MCD_CAIS_UHA_sn"
CASES = [
    ("gmm-geffner", "gmm_n300_k8", {}),
    ("gmm-dds", "gmm_n300_k8", dict(nn_arch="dds")),
    ("funnel-k16", "funnel_n300_k64", dict(nbridges=16)),
    ("many_gmm-geffner134-k6", "many_gmm_var_n16000_k256", dict(nbridges=6, init_eps=0.05)),
    ("many_gmm-dds-k12", "many_gmm_n2000_k256_dds", dict(nbridges=12, init_eps=0.05)),
]


def build(name, **over):
    return synthetic.build(name, device="cpu", dense=True, boundmode=MODE, **over)


def pieces(b):
    dim, K, mode, spec = b["params_fixed"]
    return synthetic.oracle_params(b["unflatten"], b["params_flat"]), dim, K, spec.arch, oracle_target(b["cfg"])


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_on_a_forward_path_it_is_the_forward_oracles_functional(case):
    tag, name, over = case
    b = build(name, **over)
    p, dim, K, arch, tgt = pieces(b)
    if tag.startswith("many_gmm-geffner"):
        assert p["sn"]["W1"].shape[0] == 134
    seeds = synthetic.parity_seeds(24)
    loss, zK = orc.compute_log_elbo_batch_uha(np.asarray(seeds), p, dim, K, arch, tgt, dtype=np.float64)
    path, loss_seg = rr.forward_path(seeds, p, dim, K, arch, tgt)
    assert len(path) == K + 1
    np.testing.assert_allclose(path[K][0], zK, rtol=1e-9, atol=1e-9)
    fin = np.isfinite(loss)
    assert fin.sum() >= 20
    w, z0, rho0 = rr.reverse_chain_uha(seeds, path[K][0], p, dim, K, arch, tgt, path=path)
    print(tag, "max |w + loss|", np.abs(w[fin] + loss[fin]).max(), "max |z0 - path z0|", np.abs(z0[fin] - path[0][0][fin]).max())
    np.testing.assert_allclose(w[fin], -loss[fin], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(z0[fin], path[0][0][fin], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(rho0[fin], path[0][1][fin], rtol=1e-9, atol=1e-9)


def test_one_bridge_written_out_by_hand():
    b = build("gmm_n300_k8", nbridges=1)
    p, dim, K, arch, tgt = pieces(b)
    assert K == 1
    n = 9
    seeds = synthetic.parity_seeds(n) + 7
    x = np.random.default_rng(3).normal(size=(n, dim)) * 2.0
    w, z0, rho0 = rr.reverse_chain_uha(seeds, x, p, dim, K, arch, tgt)

    vd, sn = p["vd"], p["sn"]
    beta = orc.betas_from_grid(p["mgridref_y"], p["gridref_x"], p["target_x"], np.float64)[0]
    eps = orc.eps_table(p["eps"], 1, "cos_sq", np.float64)[0]
    eta = float(p["gamma"]) * eps
    sigma = np.sqrt(2.0 * eta)
    _, b0 = prng.split(prng.prng_key(seeds))
    c, _ = prng.split(b0)
    r, g1 = prng.split(c)
    _, gen = prng.split(g1)
    g, _ = prng.split(gen)
    rho_k, xi = prng.normal(r, dim).astype(np.float64), prng.normal(g, dim).astype(np.float64)

    def log_n(v, mean, sd):
        return np.sum(-0.5 * ((v - mean) / sd) ** 2 - np.log(sd) - 0.5 * np.log(2.0 * np.pi), -1)

    def g_u(zz):
        _, gp = tgt(zz)
        return -(beta * np.clip(gp, -1e2, 1e2) + (1.0 - beta) * orc.q_grad(vd, zz))

    logp, _ = tgt(x)
    want = logp + log_n(rho_k, 0.0, 1.0)
    rho_pp = rho_k + eps * g_u(x) / 2.0
    z = x - eps * rho_pp
    rho_p = rho_pp + eps * g_u(z) / 2.0
    m_b = rho_p * (1.0 - eta) + 2.0 * eta * orc.apply_sn(arch, sn, np.concatenate([z, rho_p], 1), 0, np.float64)
    rho = m_b + sigma * xi
    m_f = rho * (1.0 - eta) - 2.0 * eta * orc.apply_sn(arch, sn, np.concatenate([z, rho], 1), 0, np.float64)
    want = want + log_n(rho, m_b, sigma) - log_n(rho_p, m_f, sigma)
    want = want - (orc.q_log_prob(vd, z) + log_n(rho, 0.0, 1.0))
    np.testing.assert_allclose(w, want, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(z0, z, rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(rho0, rho, rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize("dim,K", [(2, 8), (10, 5)])
def test_the_deviates_are_the_forward_chains_without_its_first_draw(dim, K):
    seeds = np.array([1, 2, 77, 123456, 2 ** 31 - 1], np.int32)
    _, rho0_fwd, noise = prng.particle_noise_uha(seeds, dim, K)
    rho_k, xi = rr.reverse_deviates(seeds, dim, K)
    assert np.array_equal(rho_k, rho0_fwd)          # the key the forward chain spends on rho_0
    for r in range(K):
        assert np.array_equal(xi[:, r], noise[:, r])


def test_a_non_finite_row_of_x_gives_plus_infinity_and_leaves_the_others_alone():
    b = build("gmm_n300_k8", nbridges=2)
    p, dim, K, arch, tgt = pieces(b)
    seeds = synthetic.parity_seeds(5)
    x = np.random.default_rng(1).normal(size=(5, dim))
    clean = rr.reverse_chain_uha(seeds, x, p, dim, K, arch, tgt)
    x[1, 0], x[3, 1] = np.nan, -np.inf
    w, z0, rho0 = rr.reverse_chain_uha(seeds, x, p, dim, K, arch, tgt)
    assert w[1] == np.inf and w[3] == np.inf and not np.isnan(w).any()
    for got, ref in zip((w, z0, rho0), clean):
        assert np.array_equal(got[[0, 2, 4]], ref[[0, 2, 4]])
