"""Float64 NumPy restatement of the reverse-time chain of 2nd-order CMCD (include/cmcd_hip.h: cmcd_bound_reverse_uha;
cmcd_amd/reverse_uha.py), shared by tests/test_reverse_uha_oracle.py (which pins it on the CPU against the forward oracle
compute_log_elbo_batch_uha on that oracle's own paths) and tests/test_gpu_reverse_uha.py (which holds the device to it).  Written
from the arithmetic in the header and oracle/prng.py's key functions; the pieces it calls (targets, nets, schedules, the Gaussian
log density) are oracle/'s."""
import numpy as np

from cmcd_amd import synthetic
from helpers import oracle_target
from oracle import cmcd_oracle as orc
from oracle import prng
from smc_uha_restatement import log_n01, segment_chain


def reverse_keys(seeds):
    """The forward chain's keys for MCD_CAIS_UHA_sn (oracle.prng.particle_noise_uha) without its first draw:
    (_, B) = split(PRNGKey(seed)); C = first(split(B)); (R, G') = split(C); gen_0 = second(split(G')).  -> (R, gen_0)"""
    _, b = prng.split(prng.prng_key(np.asarray(seeds)))
    c, _ = prng.split(b)
    r, g1 = prng.split(c)
    _, gen = prng.split(g1)
    return r, gen


def reverse_deviates(seeds, dim, nbridges):
    """-> (rho_K[N, dim] = normal(R), xi[N, K, dim]: reverse step r: (G, H) = split(gen), xi_r = normal(G), gen = second(split(H)))."""
    r, gen = reverse_keys(seeds)
    rho_k = prng.normal(r, dim)
    xi = np.zeros((rho_k.shape[0], nbridges, dim), np.float32)
    for step in range(nbridges):
        g, h = prng.split(gen)
        xi[:, step, :] = prng.normal(g, dim)
        _, gen = prng.split(h)
    return rho_k, xi


def _chain(seeds, x, params, dim, nbridges, arch, target, dtype, path, backward_next_index):
    dt = np.dtype(dtype).type
    p = orc.cast_params(params, dtype)
    vd, sn = p["vd"], p["sn"]
    # (the wrong chain below: row i of the rolled embedding table is row i + 1 of the real one, the last row wraps)
    sn_b = dict(sn, emb=np.roll(sn["emb"], -1, axis=0)) if backward_next_index else sn
    K = nbridges
    betas = orc.betas_from_grid(p["mgridref_y"], p["gridref_x"], p["target_x"], dtype)
    eps_tab = orc.eps_table(p["eps"], K, "cos_sq", dtype)
    gamma = dt(p["gamma"])
    clip = dt(1e2)
    one, two = dt(1.0), dt(2.0)

    def grad_u(zz, beta):
        _, gp = target(zz)
        return dt(-1.0) * (beta * np.clip(gp, -clip, clip) + (one - beta) * orc.q_grad(vd, zz))

    with np.errstate(all="ignore"):
        z = np.asarray(x, dtype).copy()
        if path is None:
            rho_k, xi = reverse_deviates(seeds, dim, K)
            rho = rho_k.astype(dtype)
        else:
            rho = np.asarray(path[K][1], dtype).copy()
        logp, _ = target(z)
        w = np.asarray(logp, dtype) + log_n01(rho)
        for i in range(K - 1, -1, -1):
            beta, eps = betas[i], eps_tab[i]
            eta = gamma * eps
            scale = np.sqrt(two * eta)
            rho_pp = rho + eps * grad_u(z, beta) / two                   # the second half-kick undone
            z = z - eps * rho_pp                                         # the drift undone
            rho_p = rho_pp + eps * grad_u(z, beta) / two                 # the first half-kick undone
            m_b = rho_p * (one - eta) + two * eta * orc.apply_sn(arch, sn_b, np.concatenate([z, rho_p], 1), i, dtype)
            dev = xi[:, K - 1 - i, :].astype(dtype) if path is None else (np.asarray(path[i][1], dtype) - m_b) / scale
            rho = m_b + scale * dev
            m_f = rho * (one - eta) - two * eta * orc.apply_sn(arch, sn, np.concatenate([z, rho], 1), i, dtype)
            w = w + (orc.log_prob_kernel(rho, m_b, scale) - orc.log_prob_kernel(rho_p, m_f, scale))
        w = w - (orc.q_log_prob(vd, z) + log_n01(rho))
        w = np.asarray(w, dtype).copy()
        w[~np.isfinite(np.asarray(x, np.float64)).all(1) | np.isnan(w)] = np.inf
    return w.astype(dtype), z.astype(dtype), rho.astype(dtype)


def reverse_chain_uha(seeds, x, params, dim, nbridges, arch, target, dtype=np.float64, path=None):
    """Per particle, with eta_i = gamma eps_i, sigma_i = sqrt(2 eta_i), gU(z, b) = -(b clip(grad log p, +-1e2) + (1 - b) grad log q):
      z_K = x; rho_K = normal(R); w = log p(z_K) + log N(rho_K; 0, I)
      for i = K-1 .. 0:  rho'' = rho_{i+1} + eps_i gU(z_{i+1}, beta_i) / 2;  z_i = z_{i+1} - eps_i rho'';
                         rho' = rho'' + eps_i gU(z_i, beta_i) / 2
                         m_b = rho' (1 - eta_i) + 2 eta_i s([z_i; rho'], i);  rho_i = m_b + sigma_i xi_r, r = K-1-i
                         m_f = rho_i (1 - eta_i) - 2 eta_i s([z_i; rho_i], i)
                         w += log N(rho_i; m_b, sigma_i) - log N(rho'; m_f, sigma_i)
      w -= log q(z_0) + log N(rho_0; 0, I)
    `path` = [(z_i, rho_i)] for i = 0 .. K (z_K = x): evaluate the functional on that path instead — rho_K is the path's, not
    normal(R), and the deviates are (rho_i - m_b) / sigma_i; the z_i are still those the inverted leap-frog produces.
    A row of x with a non-finite entry, or a NaN w, gives w = +inf.  -> (w[N], z_0[N, dim], rho_0[N, dim]) in `dtype`."""
    return _chain(seeds, x, params, dim, nbridges, arch, target, dtype, path, False)


def reverse_chain_uha_backward_at_next_index(seeds, x, params, dim, nbridges, arch, target, dtype=np.float64):
    """The WRONG chain tests/test_gpu_reverse_uha.py holds the device apart from: the backward kernel's network at index i + 1
    (the overdamped CAIS rule) instead of i.  geffner nets only (the index enters through the embedding table)."""
    return _chain(seeds, x, params, dim, nbridges, arch, target, dtype, None, True)


def forward_path(seeds, params, dim, nbridges, arch, target, dtype=np.float64):
    """[(z_i, rho_i)] for i = 0 .. K of the forward chain, and its losses: smc_uha_restatement.segment_chain one bridge at a
    time (no new forward code)."""
    state = segment_chain(np.asarray(seeds), 0, 1, params, dim, nbridges, arch, target, dtype)
    # (z_0, rho_0): a segment returns its end only, so the start is formed from the chain's first two draws as segment_chain does
    eps0, rho0, _ = prng.particle_noise_uha(np.asarray(seeds), dim, nbridges)
    z0 = orc.q_sample(orc.cast_params(params, dtype)["vd"], eps0.astype(dtype))
    path = [(z0, rho0.astype(dtype)), (state["z"], state["rho"])]
    for k in range(1, nbridges):
        state = segment_chain(state, k, k + 1, params, dim, nbridges, arch, target, dtype)
        path.append((state["z"], state["rho"]))
    return path, -(state["wpath"] + state["lg"])


# --------------------------------------------------------------------------- plumbing for synthetic.build() dicts
def run_restatement(b, seeds, x, dtype=np.float64, chain=reverse_chain_uha):
    dim, K, mode, spec = b["params_fixed"]
    assert mode == "MCD_CAIS_UHA_sn"
    return chain(seeds, x, synthetic.oracle_params(b["unflatten"], b["params_flat"]), dim, K, spec.arch, oracle_target(b["cfg"]),
                 dtype=dtype)
