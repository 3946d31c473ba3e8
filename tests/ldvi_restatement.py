"""LDVI (`MCD_U_a-lp-sn`, and `MCD_U_a-lp` without the network) restated in float64 torch: the yardstick of
tests/test_ldvi_oracle.py and tests/test_gpu_ldvi.py.

TEST INFRASTRUCTURE ONLY.  Written from /root/reference/src/mcdboundingmachine.py:126-205 (compute_log_elbo / compute_bound),
mcd_utils.py:83-120 (the dispatcher: `MCD_U_a-lp` use_sn = False, `MCD_U_a-lp-sn` use_sn = True, full_sn = True; neither takes
eps_schedule or grad_clipping) and mcd_under_lp_a.py:6-87 (evolve_underdamped_lp_a); gradients come from autograd.  Per seed, with
eta = gamma eps and sigma = sqrt(2 eta):

  (A, B) = split(PRNGKey(seed));  z = mean + exp(logdiag) normal(A);  w = -log q(z)                   mcdboundingmachine.py:151-157
  C = first(split(B));  (R, G') = split(C);  rho = normal(R);  w -= log N(rho; 0, 1);  gen = second(split(G'))    mcd_under_lp_a.py:66-74
  for i < K:  n_i from the chain;  m_f = rho (1 - eta);  rho' = m_f + sigma n_i                        :28-33
              rho'' = rho' - eps/2 gU(z, beta_i);  z' = z + eps rho'';  rho_new = rho'' - eps/2 gU(z', beta_i)    :35-37
              m_b = rho' (1 - eta) [+ 2 eta s([z; rho'], i)]                                           :40-51
              w += log N(rho; m_b, sigma) - log N(rho'; m_f, sigma);  (z, rho) = (z', rho_new)         :54-61
  w += log N(rho; 0, 1) + log p(z);  loss = -w                                                         :85, mcdboundingmachine.py:178

gU = jax.grad(U), U = -(beta log p + (1 - beta) log q): no clip.  The deviates are `oracle.prng.particle_noise_uha`'s (the key
chain of 2nd-order CMCD: initial momentum from first(split(C)), one deviate per bridge); the densities, `grad_logp` (zero where
many_gmm is floored), `_final_logp`, `apply_geffner` and `betas_from_grid` are `oracle.cmcd_oracle_torch`'s."""
import math

import numpy as np
import torch

from oracle import cmcd_oracle_torch as ot
from oracle import prng

LOG_2PI = math.log(2 * math.pi)
MODES = ("MCD_U_a-lp-sn", "MCD_U_a-lp")
SN_LEAVES = ("emb", "factor_sn", "W1", "b1", "W2", "b2", "W3", "b3")


def params_numpy(unflatten, params_flat):
    """The merged tree as float64 NumPy in the layout of oracle/cmcd_oracle.py: vd{mean, logdiag}, eps, gamma, eta, mgridref_y
    and, when the tree has a network, sn{emb, factor_sn, W1, b1, W2, b2, W3, b3} (geffner)."""
    train, notrain = unflatten(params_flat.detach().cpu())
    allp = {**train, **notrain}
    f = lambda t: np.asarray(t.numpy(), np.float64)
    out = {"vd": {k: f(v) for k, v in allp["vd"].items()}, "eps": f(allp["eps"]), "gamma": f(allp["gamma"]),
           "eta": f(allp["eta"]), "mgridref_y": f(allp["mgridref_y"])}
    if "sn" in allp:
        sn = allp["sn"]
        (w1, b1), (w2, b2), (w3, b3) = sn["nn"]
        out["sn"] = {"emb": f(sn["emb"]), "factor_sn": f(sn["factor_sn"]), "W1": f(w1), "b1": f(b1), "W2": f(w2), "b2": f(b2),
                     "W3": f(w3), "b3": f(b3)}
    return out


def leaves_of(p, prefix=()):
    """[(path, leaf)] of a nested dict, in insertion order."""
    out = []
    for k, v in p.items():
        out += leaves_of(v, prefix + (k,)) if isinstance(v, dict) else [(prefix + (k,), v)]
    return out


def log_q(vd, z):
    std = torch.exp(vd["logdiag"])
    return (-((z - vd["mean"]) ** 2) / (2 * std * std) - torch.log(std) - 0.5 * LOG_2PI).sum(-1)


def log_kernel(x, mean, scale):
    """log_prob_kernel of mcd_utils.py: independent normals of one scale."""
    return (-((x - mean) ** 2) / (2 * scale * scale) - torch.log(scale) - 0.5 * LOG_2PI).sum(-1)


def noise(seeds, dim, nbridges, dtype=torch.float64):
    e0, r0, n = prng.particle_noise_uha(np.asarray(seeds), dim, nbridges)
    t = lambda a: torch.tensor(a.astype(np.float64), dtype=dtype)
    return t(e0), t(r0), t(n)


def z0_of(p, e0):
    return torch.exp(p["vd"]["logdiag"]) * e0 + p["vd"]["mean"]


def losses(seeds, p, dim, nbridges, target, use_sn=True, create_graph=True, trace=None, local_sn=False):
    """-> (losses[N], z[N, dim]) in the dtype of `p` (an ot.to_torch dict), differentiable in its leaves.
    `trace` (a dict) receives log p BEFORE its floor at each of the K + 1 evaluations, in chain order, under "lp".
    `local_sn`: the trajectory detached — the positions, momenta and residuals enter as constants and the only path to the
    loss is s through the cotangent -(rho - m_b) / (2 eta) x 2 eta: the locality the kernels rely on for d / d sn."""
    logp_fn = ot.TARGETS[target] if isinstance(target, str) else target
    raw = getattr(logp_fn, "unfloored", logp_fn)
    vd = p["vd"]
    dt = vd["mean"].dtype
    e0, rho, n = noise(seeds, dim, nbridges, dtype=dt)
    std = torch.exp(vd["logdiag"])
    betas = ot.betas_from_grid(p["mgridref_y"], nbridges)
    eps, gamma = p["eps"], p["gamma"]
    one = torch.ones((), dtype=dt)

    def scores(z):
        """(grad log p, grad log q) at z: one target evaluation serves the kick that closes a bridge and the one that opens the next."""
        if trace is not None:
            with torch.no_grad():
                trace.setdefault("lp", []).append(raw(z.detach()).numpy().copy())
        return ot.grad_logp(logp_fn, z, create_graph=create_graph), -(z - vd["mean"]) / (std * std)

    def grad_u(gp, gq, beta):
        return -1.0 * (beta * gp + (1.0 - beta) * gq)      # jax.grad(U)(z, beta), no clip      mcd_under_lp_a.py:18-21,35

    z = z0_of(p, e0)
    w = -log_q(vd, z)
    w = w - log_kernel(rho, torch.zeros_like(rho), one)
    eta = gamma * eps
    scale = torch.sqrt(2.0 * eta)
    gp, gq = scores(z)
    for i in range(nbridges):
        beta = betas[i]
        fk = rho * (1.0 - eta)
        rho_prime = fk + scale * n[:, i, :]
        rho_pp = rho_prime - eps * grad_u(gp, gq, beta) / 2.0
        z_new = z + eps * rho_pp
        gp, gq = scores(z_new)
        rho_new = rho_pp - eps * grad_u(gp, gq, beta) / 2.0
        if local_sn:
            s = ot.apply_geffner(p["sn"], torch.cat([z.detach(), rho_prime.detach()], 1), i)
            bk = (rho_prime * (1.0 - eta)).detach() + 2.0 * eta.detach() * s
            w = w + (-((rho.detach() - bk) ** 2) / (2 * scale.detach() ** 2)).sum(-1)
        else:
            bk = rho_prime * (1.0 - eta)
            if use_sn:
                bk = bk + 2.0 * eta * ot.apply_geffner(p["sn"], torch.cat([z, rho_prime], 1), i)
            w = w + log_kernel(rho, bk, scale) - log_kernel(rho_prime, fk, scale)
        z, rho = z_new, rho_new
    w = w + log_kernel(rho, torch.zeros_like(rho), one)
    w = w + ot._final_logp(logp_fn, z, False)
    return -w, z


def _nest(paths_values):
    out = {}
    for path, v in paths_values:
        d = out
        for k in path[:-1]:
            d = d.setdefault(k, {})
        d[path[-1]] = v
    return out


def bound_and_grad(seeds, p_np, dim, nbridges, target, use_sn=True, dtype=torch.float64, local_sn=False):
    """-> (losses, z, grads) as float64 NumPy; grads = d mean(losses) / d leaf in the layout of `p_np` (what
    jax.grad(mcdbm.compute_bound, 1) returns, leaf by leaf; a leaf the loss does not read has a zero gradient).
    `dtype = torch.float32` runs the same arithmetic in single precision: only to measure what float32 alone costs on a case."""
    p = ot.to_torch(p_np, dtype=dtype)
    l, z = losses(seeds, p, dim, nbridges, target, use_sn=use_sn, local_sn=local_sn)
    lv = leaves_of(p)
    # a floored end point: the loss is +inf, its derivative that of the other terms (the floor's branch carries none)
    gs = torch.autograd.grad(l.mean(), [v for _, v in lv], allow_unused=True)
    grads = _nest((path, np.zeros(tuple(v.shape)) if g is None else g.detach().double().numpy()) for (path, v), g in zip(lv, gs))
    return l.detach().double().numpy(), z.detach().double().numpy(), grads


def forward(seeds, p_np, dim, nbridges, target, use_sn=True, trace=None, dtype=torch.float64):
    """Losses and end points without building the second-order graph."""
    p = ot.to_torch(p_np, requires_grad=False, dtype=dtype)
    with torch.enable_grad():
        l, z = losses(seeds, p, dim, nbridges, target, use_sn=use_sn, create_graph=False, trace=trace)
    return l.detach().double().numpy(), z.detach().double().numpy()


def flat_grad(unflatten, n_params, grads):
    """The gradient dict re-assembled in params_flat order (float64 torch)."""
    flat = torch.zeros(n_params, dtype=torch.float64)
    train, notrain = unflatten(flat)
    allp = {**train, **notrain}
    t = lambda a: torch.as_tensor(np.asarray(a, np.float64))
    for k in ("mean", "logdiag"):
        allp["vd"][k].copy_(t(grads["vd"][k]))
    for k in ("eps", "gamma", "eta", "mgridref_y"):
        allp[k].copy_(t(grads[k]))
    if "sn" in allp:
        sn, gs = allp["sn"], grads["sn"]
        (w1, b1), (w2, b2), (w3, b3) = sn["nn"]
        for dst, k in ((w1, "W1"), (b1, "b1"), (w2, "W2"), (b2, "b2"), (w3, "W3"), (b3, "b3")):
            dst.copy_(t(gs[k]))
        sn["emb"].copy_(t(gs["emb"]))
        sn["factor_sn"].copy_(t(gs["factor_sn"]))
    return flat


def block_errors(unflatten, flat, flat_ref):
    """{leaf name ("vd/mean", "sn/nn/0/0", ...): (max abs error, max |reference|)} over the leaves of params_train — the cut
    where different kernels write: every sn leaf, vd, eps, gamma and mgridref_y on their own."""
    out = {}
    for path, (off, shape) in unflatten.layout.items():
        if path[0] != 0:
            continue
        numel = max(1, int(np.prod(shape)))
        a, r = flat[off:off + numel].double(), flat_ref[off:off + numel].double()
        out["/".join(map(str, path[1:]))] = (float((a - r).abs().max()), float(r.abs().max()))
    return out
