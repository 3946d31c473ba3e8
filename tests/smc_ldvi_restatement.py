"""Float64 NumPy restatement of the resumable segments of LDVI (include/cmcd_hip.h: cmcd_bound_segment_ldvi; cmcd_amd/smc_ldvi.py),
shared by tests/test_smc_ldvi_hais_oracle.py (which pins it on the CPU against the forward restatement tests/ldvi_restatement.py)
and tests/test_gpu_smc_ldvi.py (which holds the device to it).  Written from the arithmetic in the header and from
tests/ldvi_restatement.py; the pieces it calls (targets, the geffner net, the beta grid, the Gaussian log densities) are oracle/'s,
the key chain is smc_uha_restatement's, and the driver and the resampling stage ARE smc_uha_restatement's (smc_chain,
resample_stage: a stage moves z and rho with the same ancestors, keys stay with their slot).

TEST INFRASTRUCTURE ONLY.  A state is a dict: z[N, d], rho[N, d], wpath[N], lg[N], key[N, 2] uint32 (gen_k), k."""
import numpy as np

from helpers import oracle_target
from oracle import cmcd_oracle as orc
from oracle import prng
from reverse_ldvi_restatement import params_numpy
from smc_uha_restatement import log_n01, losses_of, resample_stage, smc_chain  # noqa: F401  (re-exported)

MODES = ("MCD_U_a-lp-sn", "MCD_U_a-lp")


def segment_chain(state, k0, k1, params, dim, nbridges, target, use_sn=True, dtype=np.float64, trace=None):
    """Bridges [k0, k1) of LDVI.  `state` = seeds[N] at k0 == 0, else a state dict (z, rho, wpath, key; left untouched).  With
    eta = gamma eps, sigma = sqrt(2 eta), gU(z, b) = -(b grad log p + (1 - b) grad log q) (no clip):
      k0 == 0: (A, B) = split(PRNGKey(seed)); z_0 = q.sample(normal(A)); C = first(split(B)); (R, G') = split(C); rho_0 = normal(R);
               gen_0 = second(split(G')); wpath = -log q(z_0) - log N(rho_0; 0, I)
      bridge i: (G, H) = split(gen); m_f = rho (1 - eta); rho' = m_f + sigma normal(G);
               rho'' = rho' - eps gU(z, beta_i) / 2; z' = z + eps rho''; rho_new = rho'' - eps gU(z', beta_i) / 2;
               m_b = rho' (1 - eta) [+ 2 eta s([z; rho'], i)];
               wpath += log N(rho; m_b, sigma) - log N(rho'; m_f, sigma); gen = second(split(H))
      lg = log gamma_k1(z) + log N(rho; 0, I): log p(z) at k1 == K, else beta_{k1-1} log p + (1 - beta_{k1-1}) log q, and -inf
           wherever log p = -inf."""
    dt = np.dtype(dtype).type
    p = orc.cast_params(params, dtype)
    vd = p["vd"]
    sn = p["sn"] if use_sn else None
    K = nbridges
    assert 0 <= k0 < k1 <= K
    betas = orc.betas_from_grid(p["mgridref_y"], p["gridref_x"], p["target_x"], dtype)
    eps, gamma = dt(p["eps"]), dt(p["gamma"])
    one, two = dt(1.0), dt(2.0)
    eta = gamma * eps
    scale = np.sqrt(two * eta)

    unfloored = getattr(target, "unfloored", None)

    def grad_u(zz, beta):
        if trace is not None:      # log p BEFORE many_gmm's floor at every position of the segment (z_k1 is the last kick's)
            trace.setdefault("lp", []).append(np.array(unfloored(zz) if unfloored else target(zz)[0]))
        _, gp = target(zz)
        return dt(-1.0) * (beta * gp + (one - beta) * orc.q_grad(vd, zz))

    with np.errstate(all="ignore"):
        if k0 == 0:
            a, b = prng.split(prng.prng_key(np.asarray(state)))
            z = orc.q_sample(vd, prng.normal(a, dim).astype(dtype))
            c, _ = prng.split(b)
            r, g1 = prng.split(c)
            rho = prng.normal(r, dim).astype(dtype)
            _, gen = prng.split(g1)
            wpath = -orc.q_log_prob(vd, z) - log_n01(rho)
        else:
            z = np.asarray(state["z"], dtype).copy()
            rho = np.asarray(state["rho"], dtype).copy()
            wpath = np.asarray(state["wpath"], dtype).copy()
            gen = np.asarray(state["key"], np.uint32).copy()
        for i in range(k0, k1):
            beta = betas[i]
            g, h = prng.split(gen)
            m_f = rho * (one - eta)
            rho_p = m_f + scale * prng.normal(g, dim).astype(dtype)
            rho_pp = rho_p - eps * grad_u(z, beta) / two
            z_new = z + eps * rho_pp
            rho_new = rho_pp - eps * grad_u(z_new, beta) / two
            m_b = rho_p * (one - eta)
            if use_sn:
                m_b = m_b + two * eta * orc.apply_geffner(sn, np.concatenate([z, rho_p], 1), i, dtype)
            wpath = wpath + (orc.log_prob_kernel(rho, m_b, scale) - orc.log_prob_kernel(rho_p, m_f, scale))
            z, rho = z_new, rho_new
            _, gen = prng.split(h)
        logp, _ = target(z)
        lg = np.asarray(logp, dtype).copy()
        if k1 < K:
            bl = betas[k1 - 1]
            lg = np.where(logp == -np.inf, dt(-np.inf), bl * logp + (one - bl) * orc.q_log_prob(vd, z))
        lg = lg + log_n01(rho)
    return {"z": z.astype(dtype), "rho": rho.astype(dtype), "wpath": wpath.astype(dtype), "lg": lg.astype(dtype), "key": gen,
            "k": k1}


# --------------------------------------------------------------------------- plumbing for build() dicts (ldvi_cases.build's shape)
def segment_runner(b, dtype=np.float64):
    """-> run_segment(state, k0, k1) for a dict of ldvi_cases.build's shape (params_fixed carries the LDVI mode string)."""
    dim, K, mode, _ = b["params_fixed"]
    assert mode in MODES
    p, tgt = params_numpy(b["unflatten"], b["params_flat"]), oracle_target(b["cfg"])
    return lambda state, k0, k1, trace=None: segment_chain(state, k0, k1, p, dim, K, tgt, use_sn=mode == MODES[0], dtype=dtype,
                                                           trace=trace)
