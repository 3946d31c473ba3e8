"""Float64 NumPy restatement of the resumable segments of UHA, Hamiltonian AIS (include/cmcd_hip.h: cmcd_bound_segment_hais;
cmcd_amd/smc_hais.py), shared by tests/test_smc_ldvi_hais_oracle.py (which pins it on the CPU against the forward restatement
tests/hais_restatement.py) and tests/test_gpu_smc_hais.py (which holds the device to it).  Written from the arithmetic in the
header and from tests/hais_restatement.py; the targets, q and the beta grid are oracle/'s, the key chain is
smc_uha_restatement's, and the driver and the resampling stage ARE smc_uha_restatement's (smc_chain, resample_stage: a stage moves
z and rho with the same ancestors, keys stay with their slot).

TEST INFRASTRUCTURE ONLY.  A state is a dict: z[N, d], rho[N, d] (the momentum BETWEEN bridges), wpath[N], lg[N], key[N, 2]
uint32 (gen_k), k."""
import numpy as np

from oracle import cmcd_oracle as orc
from oracle import prng
from smc_uha_restatement import losses_of, resample_stage, smc_chain  # noqa: F401  (re-exported)


def segment_chain(state, k0, k1, params, dim, nbridges, lfsteps, target, dtype=np.float64, trace=None):
    """Bridges [k0, k1) of UHA.  `state` = seeds[N] at k0 == 0, else a state dict (z, rho, wpath, key; left untouched).  With
    s = exp(md), L = lfsteps, gU(z, b) = -(b grad log p + (1 - b) grad log q) (no clip):
      k0 == 0: (A, B) = split(PRNGKey(seed)); z_0 = q.sample(normal(A)); C = first(split(B)); (R, G') = split(C);
               rho_prev = s normal(R); gen_0 = second(split(G')); wpath = -log q(z_0)
      bridge i: (G, H) = split(gen); rho = eta rho_prev + sqrt(1 - eta^2) s normal(G);
               r = rho - eps/2 gU(z, beta_i); z += eps r / s^2; (L - 1) times: r -= eps gU(z, beta_i); z += eps r / s^2;
               r -= eps/2 gU(z, beta_i);  wpath += log N(r; 0, s) - log N(rho; 0, s); rho_prev = r; gen = second(split(H))
      lg = log gamma_k1(z), no momentum term: log p(z) at k1 == K, else beta_{k1-1} log p + (1 - beta_{k1-1}) log q, and -inf
           wherever log p = -inf.
    The state's rho is rho_prev."""
    dt = np.dtype(dtype).type
    p = orc.cast_params(params, dtype)
    vd = p["vd"]
    K, L = nbridges, lfsteps
    assert 0 <= k0 < k1 <= K and L >= 1
    betas = orc.betas_from_grid(p["mgridref_y"], p["gridref_x"], p["target_x"], dtype)
    eps, eta = dt(p["eps"]), dt(p["eta"])
    s = np.exp(p["md"])
    iv = dt(1.0) / (s * s)
    ce = np.sqrt(dt(1.0) - eta * eta)
    one, two = dt(1.0), dt(2.0)

    unfloored = getattr(target, "unfloored", None)

    def grad_u(zz, beta):
        if trace is not None:      # log p BEFORE many_gmm's floor at every position of the segment (z_k1 is the last kick's)
            trace.setdefault("lp", []).append(np.array(unfloored(zz) if unfloored else target(zz)[0]))
        _, gp = target(zz)
        return dt(-1.0) * (beta * gp + (one - beta) * orc.q_grad(vd, zz))

    def log_mom(rr):      # momdist.log_prob: independent normals of scale s, mean 0
        return np.sum(-(rr ** 2) / (two * s * s) - np.log(s) - dt(0.5 * orc.LOG_2PI), -1)

    with np.errstate(all="ignore"):
        if k0 == 0:
            a, b = prng.split(prng.prng_key(np.asarray(state)))
            z = orc.q_sample(vd, prng.normal(a, dim).astype(dtype))
            c, _ = prng.split(b)
            rk, g1 = prng.split(c)
            rho_prev = s * prng.normal(rk, dim).astype(dtype)
            _, gen = prng.split(g1)
            wpath = -orc.q_log_prob(vd, z)
        else:
            z = np.asarray(state["z"], dtype).copy()
            rho_prev = np.asarray(state["rho"], dtype).copy()
            wpath = np.asarray(state["wpath"], dtype).copy()
            gen = np.asarray(state["key"], np.uint32).copy()
        for i in range(k0, k1):
            beta = betas[i]
            g, h = prng.split(gen)
            rho = eta * rho_prev + ce * s * prng.normal(g, dim).astype(dtype)
            r = rho - eps * grad_u(z, beta) / two
            z = z + eps * r * iv
            for _ in range(L - 1):
                r = r - eps * grad_u(z, beta)
                z = z + eps * r * iv
            r = r - eps * grad_u(z, beta) / two
            wpath = wpath + (log_mom(r) - log_mom(rho))
            rho_prev = r
            _, gen = prng.split(h)
        logp, _ = target(z)
        lg = np.asarray(logp, dtype).copy()
        if k1 < K:
            bl = betas[k1 - 1]
            lg = np.where(logp == -np.inf, dt(-np.inf), bl * logp + (one - bl) * orc.q_log_prob(vd, z))
    return {"z": z.astype(dtype), "rho": rho_prev.astype(dtype), "wpath": wpath.astype(dtype), "lg": lg.astype(dtype), "key": gen,
            "k": k1}


# --------------------------------------------------------------------------- plumbing for hais_restatement.make_params tuples
def segment_runner(params_flat, unflatten, params_fixed, target, dtype=np.float64):
    """-> run_segment(state, k0, k1); `target` is the oracle's (helpers.oracle_target)."""
    import hais_restatement as hr
    dim, K, L = params_fixed
    p = hr.params_numpy(unflatten, params_flat)
    return lambda state, k0, k1, trace=None: segment_chain(state, k0, k1, p, dim, K, L, target, dtype=dtype, trace=trace)
