"""Float64 NumPy restatement of the resumable segments of 2nd-order CMCD (include/cmcd_hip.h: cmcd_bound_segment_uha) and of its
SMC driver (cmcd_amd/smc_uha.py), shared by tests/test_smc_uha_oracle.py (which pins it on the CPU against the forward oracle
compute_log_elbo_batch_uha) and tests/test_gpu_smc_uha.py (which holds the device to it).  Written from the arithmetic in the header
and oracle/prng.py's key chain; the pieces it calls (targets, nets, schedules, the Gaussian log density) are oracle/'s, the group
statistics and the systematic scheme are tests/smc_restatement.py's.

A state is a dict: z[N, d], rho[N, d], wpath[N], lg[N], key[N, 2] uint32 (gen_k), k."""
import numpy as np

from cmcd_amd import prng as host_prng
from cmcd_amd import synthetic
from helpers import oracle_target
from oracle import cmcd_oracle as orc
from oracle import prng
from smc_restatement import group_stats, losses_of, systematic  # noqa: F401  (losses_of: re-exported)


def log_n01(rho):
    """log N(rho; 0, I)."""
    return orc.log_prob_kernel(rho, np.zeros_like(rho), rho.dtype.type(1.0))


def segment_chain(state, k0, k1, params, dim, nbridges, arch, target, dtype=np.float64):
    """Bridges [k0, k1) of MCD_CAIS_UHA_sn.  `state` = seeds[N] at k0 == 0, else a state dict (z, rho, wpath, key; left untouched).
      k0 == 0: (A, B) = split(PRNGKey(seed)); z_0 = q.sample(normal(A)); C = first(split(B)); (R, G') = split(C); rho_0 = normal(R);
               gen_0 = second(split(G')); wpath = -log q(z_0) - log N(rho_0; 0, I)
      step i:  eta = gamma eps_i, sigma = sqrt(2 eta); (G, H) = split(gen);
               m_f = rho (1 - eta) - 2 eta s([z; rho], i); rho' = m_f + sigma normal(G);
               rho'' = rho' - eps_i gU(z, beta_i) / 2; z' = z + eps_i rho''; rho_new = rho'' - eps_i gU(z', beta_i) / 2;
               m_b = rho' (1 - eta) + 2 eta s([z; rho'], i);
               wpath += log N(rho; m_b, sigma) - log N(rho'; m_f, sigma); gen = second(split(H))
      lg = log gamma_k1(z) + log N(rho; 0, I): log p(z) at k1 == K, else beta_{k1-1} log p + (1 - beta_{k1-1}) log q, and -inf
           wherever log p = -inf."""
    dt = np.dtype(dtype).type
    p = orc.cast_params(params, dtype)
    vd, sn = p["vd"], p["sn"]
    K = nbridges
    assert 0 <= k0 < k1 <= K
    betas = orc.betas_from_grid(p["mgridref_y"], p["gridref_x"], p["target_x"], dtype)
    eps_tab = orc.eps_table(p["eps"], K, "cos_sq", dtype)
    gamma = dt(p["gamma"])
    clip = dt(1e2)

    def grad_u(zz, beta):
        _, gp = target(zz)
        return dt(-1.0) * (beta * np.clip(gp, -clip, clip) + (dt(1.0) - beta) * orc.q_grad(vd, zz))

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
            beta, eps = betas[i], eps_tab[i]
            eta = gamma * eps
            scale = np.sqrt(dt(2.0) * eta)
            g, h = prng.split(gen)
            m_f = rho * (dt(1.0) - eta) - dt(2.0) * eta * orc.apply_sn(arch, sn, np.concatenate([z, rho], 1), i, dtype)
            rho_p = m_f + scale * prng.normal(g, dim).astype(dtype)
            rho_pp = rho_p - eps * grad_u(z, beta) / dt(2.0)
            z_new = z + eps * rho_pp
            rho_new = rho_pp - eps * grad_u(z_new, beta) / dt(2.0)
            m_b = rho_p * (dt(1.0) - eta) + dt(2.0) * eta * orc.apply_sn(arch, sn, np.concatenate([z, rho_p], 1), i, dtype)
            wpath = wpath + (orc.log_prob_kernel(rho, m_b, scale) - orc.log_prob_kernel(rho_p, m_f, scale))
            z, rho = z_new, rho_new
            _, gen = prng.split(h)
        logp, _ = target(z)
        lg = np.asarray(logp, dtype).copy()
        if k1 < K:
            bl = betas[k1 - 1]
            lg = np.where(logp == -np.inf, dt(-np.inf), bl * logp + (dt(1.0) - bl) * orc.q_log_prob(vd, z))
        lg = lg + log_n01(rho)
    return {"z": z.astype(dtype), "rho": rho.astype(dtype), "wpath": wpath.astype(dtype), "lg": lg.astype(dtype), "key": gen,
            "k": k1}


def resample_stage(state, groups, ess_threshold, seed):
    """cmcd_amd.smc_uha.resample_stage in NumPy: z AND rho follow the ancestors, keys stay with their slot.
    -> (new state, resampled[groups], ess[groups], ln Z increment[groups], ancestors[N])."""
    n = state["wpath"].size
    m = n // groups
    loss = losses_of(state)
    u = host_prng.uniform(seed, (groups,), 0.0, 1.0)
    anc = np.arange(n)
    trig, ess, inc = np.zeros(groups, bool), np.zeros(groups), np.zeros(groups)
    for g in range(groups):
        sl = slice(g * m, (g + 1) * m)
        st, wn = group_stats(loss[sl])
        ess[g] = st["ess"]
        if wn is not None and st["ess"] < ess_threshold * m:
            trig[g] = True
            inc[g] = st["ln_Z"]
            anc[sl] = g * m + systematic(wn, u[g])
    new = dict(state)
    new["z"] = state["z"][anc]
    new["rho"] = state["rho"][anc]
    new["lg"] = state["lg"][anc]
    mask = np.repeat(trig, m)
    new["wpath"] = np.where(mask, -state["lg"][anc], state["wpath"])
    return new, trig, ess, inc, anc


def smc_chain(seeds, run_segment, nbridges, groups=1, cuts=None, ess_threshold=0.5, seed=0):
    """cmcd_amd.smc_uha.smc_bound in NumPy; run_segment(state, k0, k1) -> state.
    -> dict(ln_Z, losses, z, rho, resampled, ess, ancestors, state, arrived: the states as they arrived at each cut)."""
    K = nbridges
    if cuts is None:
        step = max(1, K // 8)
        cuts = list(range(step, K, step))
    edges = list(cuts) + [K]
    state = run_segment(np.asarray(seeds), 0, edges[0])
    n = state["wpath"].size
    m = n // groups
    ln_z = np.zeros(groups)
    resampled, ess, ancestors, arrived = [], [], [], []
    for c, nxt in zip(cuts, edges[1:]):
        arrived.append(state)
        state, trig, e, inc, anc = resample_stage(state, groups, ess_threshold, seed + c)
        ln_z += inc
        resampled.append(trig)
        ess.append(e)
        ancestors.append(anc)
        state = run_segment(state, c, nxt)
    loss = losses_of(state)
    final = [group_stats(loss[g * m:(g + 1) * m])[0] for g in range(groups)]
    ess.append(np.array([f["ess"] for f in final]))
    with np.errstate(all="ignore"):
        ln_z = ln_z + np.array([f["ln_Z"] for f in final])
    return dict(ln_Z=ln_z, losses=loss, z=state["z"], rho=state["rho"], resampled=np.array(resampled).reshape(len(cuts), groups),
                ess=np.array(ess), ancestors=ancestors, state=state, arrived=arrived)


# --------------------------------------------------------------------------- plumbing for synthetic.build() dicts
def segment_runner(b):
    """-> run_segment(state, k0, k1) for a synthetic.build() dict in mode MCD_CAIS_UHA_sn, in float64."""
    dim, K, mode, spec = b["params_fixed"]
    assert mode == "MCD_CAIS_UHA_sn"
    p, tgt = synthetic.oracle_params(b["unflatten"], b["params_flat"]), oracle_target(b["cfg"])
    return lambda state, k0, k1: segment_chain(state, k0, k1, p, dim, K, spec.arch, tgt)
