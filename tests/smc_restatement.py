"""Float64 NumPy restatement of the resumable chain segments (include/cmcd_hip.h: cmcd_bound_segment) and of the SMC driver
(cmcd_amd/smc.py), shared by tests/test_smc_oracle.py (which pins it on the CPU against the forward oracle) and
tests/test_gpu_smc.py (which holds the device to it).  Written from the arithmetic in the header and oracle/prng.py's key
chain; the pieces it calls (targets, nets, schedules, the Gaussian log density) are oracle/'s.

A state is a dict: z[N, d], wpath[N], lg[N], key[N, 2] uint32 (gen_k), k."""
import math

import numpy as np

from cmcd_amd import prng as host_prng
from cmcd_amd import synthetic
from helpers import oracle_target
from oracle import cmcd_oracle as orc
from oracle import prng


def segment_chain(state, k0, k1, params, dim, nbridges, mode, arch, target, eps_schedule=None, grad_clipping=False,
                  dtype=np.float64):
    """Bridges [k0, k1).  `state` = seeds[N] at k0 == 0, else a state dict (z, wpath, key; left untouched).
      k0 == 0: (A, B) = split(PRNGKey(seed)); z_0 = q.sample(normal(A)); wpath = -log q(z_0); gen_0 = second(split(first(split(B))))
      step i:  (G, H) = split(gen); z' = m_f(z, i) + sigma_i normal(G); wpath += log N(z; m_b(z', i), sigma_i) - log N(z'; m_f, sigma_i);
               gen = second(split(H))
      lg = log p(z) at k1 == K, else beta_{k1-1} log p + (1 - beta_{k1-1}) log q, and -inf wherever log p = -inf."""
    dt = np.dtype(dtype).type
    p = orc.cast_params(params, dtype)
    vd, sn = p["vd"], p.get("sn")
    K = nbridges
    assert 0 <= k0 < k1 <= K
    betas = orc.betas_from_grid(p["mgridref_y"], p["gridref_x"], p["target_x"], dtype)
    ula = mode in ("MCD_ULA", "MCD_ULA_sn")
    eps_tab = np.full(K, dt(p["eps"]), dtype) if ula else orc.eps_table(p["eps"], K, eps_schedule, dtype)
    clipping = bool(grad_clipping) and not ula
    var_mode = mode == "MCD_CAIS_var_sn"
    clip = dt(1e2) if var_mode else dt(1e3)

    def grad_u(zz, beta):
        _, gp = target(zz)
        gq = orc.q_grad(vd, zz)
        if clipping:
            gp = np.clip(gp, -clip, clip)
            if var_mode:
                gq = np.clip(gq, -clip, clip)
        return dt(-1.0) * (beta * gp + (dt(1.0) - beta) * gq)

    with np.errstate(all="ignore"):
        if k0 == 0:
            a, b = prng.split(prng.prng_key(np.asarray(state)))
            z = orc.q_sample(vd, prng.normal(a, dim).astype(dtype))
            wpath = -orc.q_log_prob(vd, z)
            c, _ = prng.split(b)
            _, gen = prng.split(c)
        else:
            z = np.asarray(state["z"], dtype).copy()
            wpath = np.asarray(state["wpath"], dtype).copy()
            gen = np.asarray(state["key"], np.uint32).copy()
        for i in range(k0, k1):
            beta, eps = betas[i], eps_tab[i]
            scale = np.sqrt(dt(2.0) * eps)
            g, h = prng.split(gen)
            m_f = z - eps * grad_u(z, beta)
            if not ula:
                m_f = m_f - eps * orc.apply_sn(arch, sn, z, i, dtype)
            z_new = m_f + scale * prng.normal(g, dim).astype(dtype)
            m_b = z_new - eps * grad_u(z_new, beta)
            if mode != "MCD_ULA":
                m_b = m_b + eps * orc.apply_sn(arch, sn, z_new, i if ula else i + 1, dtype)
            wpath = wpath + (orc.log_prob_kernel(z, m_b, scale) - orc.log_prob_kernel(z_new, m_f, scale))
            z = z_new
            _, gen = prng.split(h)
        logp, _ = target(z)
        lg = np.asarray(logp, dtype).copy()
        if k1 < K:
            bl = betas[k1 - 1]
            lg = np.where(logp == -np.inf, dt(-np.inf), bl * logp + (dt(1.0) - bl) * orc.q_log_prob(vd, z))
    return {"z": z.astype(dtype), "wpath": wpath.astype(dtype), "lg": lg.astype(dtype), "key": gen, "k": k1}


def losses_of(state):
    with np.errstate(all="ignore"):
        return -(state["wpath"] + state["lg"])


def group_stats(loss):
    """One group's {n_finite, ln Z, ESS, diverged} and normalised weights (None when diverged or without a finite loss), as
    include/cmcd_hip.h describes cmcd_resample_systematic: float64, M = max(-loss) over the finite entries."""
    l = np.asarray(loss, np.float64)
    m = l.size
    if np.isnan(l).any() or (l == -np.inf).any():
        return dict(n_finite=np.nan, ln_Z=np.nan, ess=np.nan, diverged=1.0), None
    fin = np.isfinite(l)
    if not fin.any():
        return dict(n_finite=0.0, ln_Z=-np.inf, ess=0.0, diverged=0.0), None
    M = (-l[fin]).max()
    w = np.exp(-l - M)
    s1, s2 = w.sum(), (w * w).sum()
    return dict(n_finite=float(fin.sum()), ln_Z=M + math.log(s1) - math.log(m), ess=s1 * s1 / s2, diverged=0.0), w / s1


def systematic(wn, u):
    """Ancestors of one group: thresholds (k + u) / m against the inclusive cumulative sum, never past the last positive weight."""
    m = wn.size
    a = np.searchsorted(np.cumsum(wn), (np.arange(m) + np.float64(u)) / m, side="right")
    return np.minimum(a, np.flatnonzero(wn > 0)[-1])


def resample_stage(state, groups, ess_threshold, seed):
    """cmcd_amd.smc.resample_stage in NumPy.  -> (new state, resampled[groups], ess[groups], ln Z increment[groups], ancestors[N])."""
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
    new["lg"] = state["lg"][anc]
    mask = np.repeat(trig, m)
    new["wpath"] = np.where(mask, -state["lg"][anc], state["wpath"])
    return new, trig, ess, inc, anc


def smc_chain(seeds, run_segment, nbridges, groups=1, cuts=None, ess_threshold=0.5, seed=0):
    """cmcd_amd.smc.smc_bound in NumPy; run_segment(state, k0, k1) -> state.  -> dict(ln_Z, losses, z, resampled, ess, ancestors)."""
    K = nbridges
    if cuts is None:
        step = max(1, K // 8)
        cuts = list(range(step, K, step))
    edges = list(cuts) + [K]
    state = run_segment(np.asarray(seeds), 0, edges[0])
    n = state["wpath"].size
    m = n // groups
    ln_z = np.zeros(groups)
    resampled, ess, ancestors = [], [], []
    for c, nxt in zip(cuts, edges[1:]):
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
    return dict(ln_Z=ln_z, losses=loss, z=state["z"], resampled=np.array(resampled).reshape(len(cuts), groups),
                ess=np.array(ess), ancestors=ancestors, state=state)


# --------------------------------------------------------------------------- plumbing for synthetic.build() dicts
def oracle_params(b):
    """synthetic.oracle_params, also for MCD_ULA (whose parameter tree keeps no network)."""
    if b["params_fixed"][2] != "MCD_ULA":
        return synthetic.oracle_params(b["unflatten"], b["params_flat"])
    train, notrain = b["unflatten"](b["params_flat"].detach().cpu())
    allp = {**train, **notrain}
    f = lambda t: np.asarray(t.numpy(), np.float64)
    return {"vd": {k: f(v) for k, v in allp["vd"].items()}, "eps": f(allp["eps"]), "mgridref_y": f(allp["mgridref_y"]),
            "gridref_x": f(allp["gridref_x"]), "target_x": f(allp["target_x"])}


def segment_runner(b):
    """-> run_segment(state, k0, k1) for a synthetic.build() dict, in float64."""
    dim, K, mode, spec = b["params_fixed"]
    arch = spec.arch if spec is not None else "dds"
    p, tgt, cfg = oracle_params(b), oracle_target(b["cfg"]), b["cfg"]
    return lambda state, k0, k1: segment_chain(state, k0, k1, p, dim, K, mode, arch, tgt, eps_schedule=cfg["eps_schedule"],
                                               grad_clipping=cfg["grad_clipping"])
