"""Float64 NumPy restatement of the reverse-time chain of LDVI (include/cmcd_hip.h: cmcd_bound_reverse_ldvi;
cmcd_amd/reverse_ldvi.py), shared by tests/test_reverse_ldvi_oracle.py (which pins it on the CPU against the forward restatement
tests/ldvi_restatement.py on that restatement's own paths) and tests/test_gpu_reverse_ldvi.py (which holds the device to it).
Written from the arithmetic in the header and reverse_uha_restatement's key functions; the pieces it calls (targets, the geffner
net, the beta grid, the Gaussian log densities) are oracle/'s.

TEST INFRASTRUCTURE ONLY.  Besides the chain it holds two deliberately WRONG chains the tests keep the device apart from."""
import numpy as np

from helpers import oracle_target
from oracle import cmcd_oracle as orc
from oracle import prng
from reverse_uha_restatement import reverse_deviates
from smc_uha_restatement import log_n01


def params_numpy(unflatten, params_flat):
    """The merged tree as float64 NumPy: vd{mean, logdiag}, eps, gamma, mgridref_y, gridref_x, target_x and, when the tree has a
    network, sn{emb, factor_sn, W1, b1, W2, b2, W3, b3} (geffner)."""
    train, notrain = unflatten(params_flat.detach().cpu())
    allp = {**train, **notrain}
    f = lambda t: np.asarray(t.numpy(), np.float64)
    out = {"vd": {k: f(v) for k, v in allp["vd"].items()}}
    for k in ("eps", "gamma", "mgridref_y", "gridref_x", "target_x"):
        out[k] = f(allp[k])
    if "sn" in allp:
        sn = allp["sn"]
        (w1, b1), (w2, b2), (w3, b3) = sn["nn"]
        out["sn"] = {"emb": f(sn["emb"]), "factor_sn": f(sn["factor_sn"]), "W1": f(w1), "b1": f(b1), "W2": f(w2), "b2": f(b2),
                     "W3": f(w3), "b3": f(b3)}
    return out


def _chain(seeds, x, params, dim, nbridges, target, use_sn, dtype, path, wrong, trace=None):
    dt = np.dtype(dtype).type
    p = orc.cast_params(params, dtype)
    vd = p["vd"]
    sn = p["sn"] if use_sn else None
    # (wrong chain "next_index": row i of the rolled embedding table is row i + 1 of the real one, the last row wraps)
    sn_b = dict(sn, emb=np.roll(sn["emb"], -1, axis=0)) if (use_sn and wrong == "next_index") else sn
    K = nbridges
    betas = orc.betas_from_grid(p["mgridref_y"], p["gridref_x"], p["target_x"], dtype)
    eps, gamma = dt(p["eps"]), dt(p["gamma"])
    one, two = dt(1.0), dt(2.0)
    eta = gamma * eps
    scale = np.sqrt(two * eta)
    unfloored = getattr(target, "unfloored", None)

    def scores(zz):            # ONE target evaluation per state, as in the kernel
        if trace is not None:
            trace.setdefault("lp", []).append(np.array(unfloored(zz) if unfloored else target(zz)[0]))
        logp, gp = target(zz)
        return logp, gp, orc.q_grad(vd, zz)

    def grad_u(gp, gq, beta):  # no clip
        return dt(-1.0) * (beta * gp + (one - beta) * gq)

    with np.errstate(all="ignore"):
        z = np.asarray(x, dtype).copy()
        if path is None:
            rho_k, xi = reverse_deviates(seeds, dim, K)
            rho = rho_k.astype(dtype)
        else:
            rho = np.asarray(path[K][1], dtype).copy()
        logp, gp, gq = scores(z)
        w = np.asarray(logp, dtype) + log_n01(rho)
        floored = np.isneginf(np.asarray(logp, np.float64))
        for i in range(K - 1, -1, -1):
            beta = betas[i]
            rho_pp = rho + eps * grad_u(gp, gq, beta) / two              # the closing half-kick undone
            z = z - eps * rho_pp                                         # the drift undone
            _, gp, gq = scores(z)
            gz = grad_u(gp, gq, beta)
            rho_p = rho_pp + eps * gz / two                              # the opening half-kick undone
            m_b = rho_p * (one - eta)
            if use_sn:
                m_b = m_b + two * eta * orc.apply_geffner(sn_b, np.concatenate([z, rho_p], 1), i, dtype)
            dev = xi[:, K - 1 - i, :].astype(dtype) if path is None else (np.asarray(path[i][1], dtype) - m_b) / scale
            rho = m_b + scale * dev
            m_f = rho * (one - eta)
            if use_sn and wrong == "forward_net":                         # the 2nd-order rule: a forward mean with the network
                m_f = m_f - two * eta * orc.apply_geffner(sn, np.concatenate([z, rho], 1), i, dtype)
            w = w + (orc.log_prob_kernel(rho, m_b, scale) - orc.log_prob_kernel(rho_p, m_f, scale))
        w = w - (orc.q_log_prob(vd, z) + log_n01(rho))
        w = np.asarray(w, dtype).copy()
        w[~np.isfinite(np.asarray(x, np.float64)).all(1) | floored | np.isnan(w)] = np.inf
    return w.astype(dtype), z.astype(dtype), rho.astype(dtype)


def reverse_chain_ldvi(seeds, x, params, dim, nbridges, target, use_sn=True, dtype=np.float64, path=None, trace=None):
    """Per particle, with eta = gamma eps, sigma = sqrt(2 eta), gU(z, b) = -(b grad log p + (1 - b) grad log q) (no clip):
      z_K = x; rho_K = normal(R); w = log p(z_K) + log N(rho_K; 0, I)
      for i = K-1 .. 0:  rho'' = rho_{i+1} + eps gU(z_{i+1}, beta_i) / 2;  z_i = z_{i+1} - eps rho'';
                         rho' = rho'' + eps gU(z_i, beta_i) / 2
                         m_b = rho' (1 - eta) [+ 2 eta s([z_i; rho'], i)];  rho_i = m_b + sigma xi_r, r = K-1-i
                         m_f = rho_i (1 - eta)
                         w += log N(rho_i; m_b, sigma) - log N(rho'; m_f, sigma)
      w -= log q(z_0) + log N(rho_0; 0, I)
    `path` = [(z_i, rho_i)] for i = 0 .. K (z_K = x): evaluate the functional on that path instead — rho_K is the path's, not
    normal(R), and the deviates are (rho_i - m_b) / sigma; the z_i are still those the inverted leap-frog produces.
    `trace` (a dict) receives under "lp" log p BEFORE many_gmm's floor at z_K, z_{K-1}, .., z_0 (K + 1 arrays).
    A row of x with a non-finite entry, a floored log p(x), or a NaN w, gives w = +inf.  -> (w[N], z_0[N, dim], rho_0[N, dim])."""
    return _chain(seeds, x, params, dim, nbridges, target, use_sn, dtype, path, None, trace)


def reverse_chain_ldvi_backward_at_next_index(seeds, x, params, dim, nbridges, target, dtype=np.float64):
    """WRONG: the backward network at index i + 1 (the overdamped CAIS rule), by the rolled embedding table."""
    return _chain(seeds, x, params, dim, nbridges, target, True, dtype, None, "next_index")


def reverse_chain_ldvi_forward_mean_with_network(seeds, x, params, dim, nbridges, target, dtype=np.float64):
    """WRONG: m_f = rho_i (1 - eta) - 2 eta s([z_i; rho_i], i), the 2nd-order CMCD rule; LDVI's forward kernel has no network."""
    return _chain(seeds, x, params, dim, nbridges, target, True, dtype, None, "forward_net")


def forward_path(seeds, params, dim, nbridges, target, dtype=np.float64):
    """[(z_i, rho_i)] for i = 0 .. K of LDVI's forward chain (tests/ldvi_restatement.py's arithmetic for the positions and momenta:
    they do not depend on the network), from oracle.prng.particle_noise_uha's deviates."""
    dt = np.dtype(dtype).type
    p = orc.cast_params(params, dtype)
    vd = p["vd"]
    betas = orc.betas_from_grid(p["mgridref_y"], p["gridref_x"], p["target_x"], dtype)
    eps, gamma = dt(p["eps"]), dt(p["gamma"])
    eta = gamma * eps
    scale = np.sqrt(dt(2.0) * eta)
    e0, r0, n = prng.particle_noise_uha(np.asarray(seeds), dim, nbridges)
    z = orc.q_sample(vd, e0.astype(dtype))
    rho = r0.astype(dtype)
    path = [(z, rho)]

    def grad_u(zz, beta):
        _, gp = target(zz)
        return dt(-1.0) * (beta * gp + (dt(1.0) - beta) * orc.q_grad(vd, zz))

    for i in range(nbridges):
        rho_p = rho * (dt(1.0) - eta) + scale * n[:, i, :].astype(dtype)
        rho_pp = rho_p - eps * grad_u(z, betas[i]) / dt(2.0)
        z = z + eps * rho_pp
        rho = rho_pp - eps * grad_u(z, betas[i]) / dt(2.0)
        path.append((z, rho))
    return path


# --------------------------------------------------------------------------- plumbing for build() dicts (ldvi_cases.build's shape)
def run_restatement(b, seeds, x, dtype=np.float64, chain=reverse_chain_ldvi, **kw):
    dim, K, mode, _ = b["params_fixed"]
    assert mode in ("MCD_U_a-lp-sn", "MCD_U_a-lp")
    if chain is reverse_chain_ldvi:
        kw = dict(kw, use_sn=mode == "MCD_U_a-lp-sn")
    return chain(seeds, x, params_numpy(b["unflatten"], b["params_flat"]), dim, K, oracle_target(b["cfg"]), dtype=dtype, **kw)
