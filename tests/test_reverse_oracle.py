"""Pins `reverse_chain` (tests/test_gpu_reverse.py), the float64 restatement the reverse-time kernel is held to, without a
device: against the forward oracle on the forward oracle's own paths, by hand for one bridge, and against the longhand
ULA-AIS backward sampler."""
import numpy as np
import pytest

from cmcd_amd import synthetic
from helpers import oracle_target
from oracle import cmcd_oracle as orc
from oracle import prng
from test_gpu_reverse import reverse_chain


def forward_path(seeds, p, dim, K, mode, arch, target, eps_schedule, grad_clipping):
    """z_0 .. z_K of the forward chain in float64, in the forward oracle's own order of operations (its result is compared
    with the oracle's z_K by the caller)."""
    vd, sn = p["vd"], p.get("sn")
    e0, noise = prng.particle_noise(seeds, dim, K)
    betas = orc.betas_from_grid(p["mgridref_y"], p["gridref_x"], p["target_x"], np.float64)
    ula = mode in ("MCD_ULA", "MCD_ULA_sn")
    eps_tab = orc.eps_table(p["eps"], K, None if ula else eps_schedule, np.float64)
    clip = 1e2 if mode == "MCD_CAIS_var_sn" else 1e3
    z = orc.q_sample(vd, e0.astype(np.float64))
    path = [z]
    for i in range(K):
        _, gp = target(z)
        gq = orc.q_grad(vd, z)
        if grad_clipping and not ula:
            gp = np.clip(gp, -clip, clip)
            if mode == "MCD_CAIS_var_sn":
                gq = np.clip(gq, -clip, clip)
        uf = -1.0 * (betas[i] * gp + (1.0 - betas[i]) * gq)
        mean = z - eps_tab[i] * uf
        if not ula:
            mean = mean - eps_tab[i] * orc.apply_sn(arch, sn, z, i, np.float64)
        z = mean + np.sqrt(2.0 * eps_tab[i]) * noise[:, i, :].astype(np.float64)
        path.append(z)
    return path


@pytest.mark.parametrize("name,over", [
    ("gmm_n300_k8", {}),
    ("gmm_n300_k8", dict(boundmode="MCD_ULA_sn")),
    ("gmm_n300_k8", dict(nn_arch="dds", eps_schedule="linear", grad_clipping=True)),
    ("funnel_n300_k64", dict(nbridges=16)),
    ("many_gmm_var_n16000_k256", dict(nbridges=6)),
    ("many_gmm_n2000_k256_dds", dict(nbridges=12)),
])
def test_on_a_forward_path_the_functional_is_the_forward_weight(name, over):
    """w_reverse(path) == -loss_forward(path) when the reverse deviates are the path's own increments."""
    b = synthetic.build(name, device="cpu", dense=True, **over)
    dim, K, mode, spec = b["params_fixed"]
    cfg = b["cfg"]
    p = synthetic.oracle_params(b["unflatten"], b["params_flat"])
    tgt = oracle_target(cfg)
    seeds = synthetic.parity_seeds(24)
    loss, zK = orc.compute_log_elbo_batch(seeds, p, dim, K, mode, spec.arch, tgt, eps_schedule=cfg["eps_schedule"],
                                          grad_clipping=cfg["grad_clipping"], dtype=np.float64)
    path = forward_path(seeds, p, dim, K, mode, spec.arch, tgt, cfg["eps_schedule"], cfg["grad_clipping"])
    np.testing.assert_allclose(path[-1], zK, rtol=1e-12, atol=1e-12)
    w, z0 = reverse_chain(seeds, path[-1], p, dim, K, mode, spec.arch, tgt, eps_schedule=cfg["eps_schedule"],
                          grad_clipping=cfg["grad_clipping"], path=path)
    fin = np.isfinite(loss)
    assert fin.sum() >= 20
    np.testing.assert_allclose(z0[fin], path[0][fin], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(w[fin], -loss[fin], rtol=1e-9, atol=1e-9)


def test_one_bridge_by_hand():
    b = synthetic.build("gmm_n300_k8", device="cpu", dense=True, nbridges=1)
    p = synthetic.oracle_params(b["unflatten"], b["params_flat"])
    tgt = oracle_target(b["cfg"])
    seeds = synthetic.parity_seeds(9)
    x = np.random.default_rng(0).normal(size=(9, 2)) * 2.0
    w, z0 = reverse_chain(seeds, x, p, 2, 1, "MCD_CAIS_sn", "geffner", tgt)

    vd, sn, eps = p["vd"], p["sn"], float(p["eps"])
    beta = float(orc.betas_from_grid(p["mgridref_y"], p["gridref_x"], p["target_x"], np.float64)[0])
    sig = np.sqrt(2.0 * eps)
    _, xi = prng.particle_noise(seeds, 2, 1)
    lp1, gp1 = tgt(x)
    m_b = x + eps * (beta * gp1 + (1 - beta) * orc.q_grad(vd, x)) + eps * orc.apply_geffner(sn, x, 1, np.float64)
    z = m_b + sig * xi[:, 0, :]
    _, gp0 = tgt(z)
    m_f = z + eps * (beta * gp0 + (1 - beta) * orc.q_grad(vd, z)) - eps * orc.apply_geffner(sn, z, 0, np.float64)
    log_n = lambda y, m: np.sum(-((y - m) ** 2) / (2 * sig * sig) - np.log(sig) - 0.5 * np.log(2 * np.pi), -1)
    want = lp1 + log_n(z, m_b) - log_n(x, m_f) - orc.q_log_prob(vd, z)
    np.testing.assert_allclose(z0, z, rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(w, want, rtol=1e-12, atol=1e-12)


def test_zero_network_is_the_ula_ais_backward_sampler():
    b = synthetic.build("gmm_n300_k8", device="cpu", dense=True)
    p = synthetic.oracle_params(b["unflatten"], b["params_flat"])
    tgt = oracle_target(b["cfg"])
    K, n = 8, 31
    seeds = synthetic.parity_seeds(n)
    x = np.random.default_rng(1).normal(size=(n, 2)) * 1.5 + np.array([2.0, 1.0])
    p0 = dict(p, sn=dict(p["sn"], factor_sn=np.zeros(())))
    w_cais, z_cais = reverse_chain(seeds, x, p0, 2, K, "MCD_CAIS_sn", "geffner", tgt)
    w_ula, z_ula = reverse_chain(seeds, x, {k: v for k, v in p.items() if k != "sn"}, 2, K, "MCD_ULA", "dds", tgt,
                                 eps_schedule="cos_sq", grad_clipping=True)     # both ignored, as in the forward call

    # longhand: unadjusted Langevin on pi_beta = p^beta q^(1 - beta), run from beta_{K-1} down to beta_0
    vd, eps = p["vd"], float(p["eps"])
    betas = orc.betas_from_grid(p["mgridref_y"], p["gridref_x"], p["target_x"], np.float64)
    _, xi = prng.particle_noise(seeds, 2, K)
    score = lambda y, bt: bt * tgt(y)[1] + (1 - bt) * orc.q_grad(vd, y)
    log_n = lambda y, m: np.sum(-((y - m) ** 2) / (4 * eps) - 0.5 * np.log(4 * np.pi * eps), -1)
    z, w = x.copy(), tgt(x)[0].copy()
    for r, i in enumerate(range(K - 1, -1, -1)):
        mean_b = z + eps * score(z, betas[i])
        z_new = mean_b + np.sqrt(2 * eps) * xi[:, r, :]
        w += log_n(z_new, mean_b) - log_n(z, z_new + eps * score(z_new, betas[i]))
        z = z_new
    w -= orc.q_log_prob(vd, z)
    for got_w, got_z in ((w_cais, z_cais), (w_ula, z_ula)):
        np.testing.assert_allclose(got_z, z, rtol=1e-11, atol=1e-11)
        np.testing.assert_allclose(got_w, w, rtol=1e-11, atol=1e-10)


def test_non_finite_rows_map_to_plus_inf():
    b = synthetic.build("gmm_n300_k8", device="cpu", nbridges=2)
    p = synthetic.oracle_params(b["unflatten"], b["params_flat"])
    x = np.zeros((3, 2))
    x[0, 1], x[2, 0] = np.nan, np.inf
    w, _ = reverse_chain(np.arange(1, 4), x, p, 2, 2, "MCD_CAIS_sn", "geffner", oracle_target(b["cfg"]))
    assert w[0] == np.inf and w[2] == np.inf and np.isfinite(w[1])
