"""UHA (Hamiltonian AIS) restated in float64 torch: the yardstick of tests/test_hais_oracle.py and tests/test_gpu_hais.py.

TEST INFRASTRUCTURE ONLY.  Written from /root/reference/src/boundingmachine.py:73-111 (compute_log_elbo / compute_bound),
ais_utils.py:7-69 (evolve, leapfrog) and momdist.py:13-28 (sample, log_prob); gradients come from autograd.  Per seed, with
s = exp(md), L = lfsteps:

  (A, B) = split(PRNGKey(seed));  z = mean + exp(logdiag) normal(A);  w = -log q(z)
  C = first(split(B));  (R, G') = split(C);  rho_prev = s normal(R);  gen = second(split(G'))
  for i < K:  xi_i from the chain;  rho = eta rho_prev + sqrt(1 - eta^2) s xi_i;  (z, r) = leapfrog(z, rho, beta_i)
              w += log N(r; 0, s) - log N(rho; 0, s);  rho_prev = r
  w += log p(z);  loss = -w

The deviates are `oracle.prng.particle_noise_uha`'s (the same key chain: initial momentum from first(split(C)), one deviate per
bridge), the densities and the beta grid `oracle.cmcd_oracle_torch`'s.  delta_H is dropped (compute_bound drops it)."""
import math

import numpy as np
import torch

from oracle import cmcd_oracle_torch as ot
from oracle import prng

LOG_2PI = math.log(2 * math.pi)


def params_numpy(unflatten, params_flat):
    """The merged tree {**params_train, **params_notrain} as float64 NumPy: vd{mean, logdiag}, eps, eta, md, mgridref_y, ..."""
    train, notrain = unflatten(params_flat.detach().cpu())
    allp = {**train, **notrain}
    f = lambda t: np.asarray(t.numpy(), np.float64)
    return {k: ({kk: f(vv) for kk, vv in v.items()} if isinstance(v, dict) else f(v)) for k, v in allp.items()}


LEAVES = (("vd", "mean"), ("vd", "logdiag"), ("eps",), ("eta",), ("md",), ("mgridref_y",))


def to_torch(p, requires_grad=True):
    """float64 torch leaves of the six differentiable leaves (the two grids are not needed: both are uniform)."""
    t = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=torch.float64).requires_grad_(requires_grad)
    return {"vd": {"mean": t(p["vd"]["mean"]), "logdiag": t(p["vd"]["logdiag"])}, "eps": t(p["eps"]), "eta": t(p["eta"]),
            "md": t(p["md"]), "mgridref_y": t(p["mgridref_y"])}


def leaf(p, path):
    for k in path:
        p = p[k]
    return p


def log_q(vd, z):
    std = torch.exp(vd["logdiag"])
    return (-((z - vd["mean"]) ** 2) / (2 * std * std) - torch.log(std) - 0.5 * LOG_2PI).sum(-1)


def log_mom(md, rho):
    """momdist.log_prob: independent normals of scale exp(md), mean 0."""
    s = torch.exp(md)
    return (-(rho ** 2) / (2 * s * s) - torch.log(s) - 0.5 * LOG_2PI).sum(-1)


def grad_u(p, logp_fn, z, beta, create_graph=True):
    """jax.grad(U)(z, beta), U = -(beta log p + (1 - beta) log q)      ais_utils.py:8-9 (no clip in this mode)."""
    std = torch.exp(p["vd"]["logdiag"])
    gq = -(z - p["vd"]["mean"]) / (std * std)
    gp = ot.grad_logp(logp_fn, z, create_graph=create_graph)
    return -1.0 * (beta * gp + (1.0 - beta) * gq)


def leapfrog(p, logp_fn, z, rho, beta, lfsteps, create_graph=True):
    """ais_utils.py:26-57 without delta_H; grad K(rho) = rho / s^2."""
    eps, iv = p["eps"], torch.exp(-2.0 * p["md"])
    rho = rho - eps * grad_u(p, logp_fn, z, beta, create_graph) / 2.0
    z = z + eps * rho * iv
    for _ in range(lfsteps - 1):
        rho = rho - eps * grad_u(p, logp_fn, z, beta, create_graph)
        z = z + eps * rho * iv
    rho = rho - eps * grad_u(p, logp_fn, z, beta, create_graph) / 2.0
    return z, rho


def noise(seeds, dim, nbridges):
    e0, n0, xi = prng.particle_noise_uha(np.asarray(seeds), dim, nbridges)
    t = lambda a: torch.tensor(a.astype(np.float64))
    return t(e0), t(n0), t(xi)


def z0_of(p, e0):
    return torch.exp(p["vd"]["logdiag"]) * e0 + p["vd"]["mean"]


def losses(seeds, p, dim, nbridges, lfsteps, target, create_graph=True):
    """-> (losses[N], z[N, dim]) float64, differentiable in the leaves of `p` (a to_torch dict)."""
    logp_fn = ot.TARGETS[target] if isinstance(target, str) else target
    e0, n0, xi = noise(seeds, dim, nbridges)
    s = torch.exp(p["md"])
    z = z0_of(p, e0)
    w = -log_q(p["vd"], z)
    if nbridges >= 1:
        betas = ot.betas_from_grid(p["mgridref_y"], nbridges)
        rho_prev = s * n0
        for i in range(nbridges):
            rho = p["eta"] * rho_prev + torch.sqrt(1.0 - p["eta"] ** 2) * s * xi[:, i, :]
            z, r = leapfrog(p, logp_fn, z, rho, betas[i], lfsteps, create_graph)
            w = w + log_mom(p["md"], r) - log_mom(p["md"], rho)
            rho_prev = r
    w = w + logp_fn(z)
    return -w, z


def bound_and_grad(seeds, p_np, dim, nbridges, lfsteps, target):
    """-> (losses, z, {leaf path: d mean(losses) / d leaf}) as NumPy; what jax.grad(bm.compute_bound, 1) returns, leaf by leaf."""
    p = to_torch(p_np)
    l, z = losses(seeds, p, dim, nbridges, lfsteps, target)
    gs = torch.autograd.grad(l.mean(), [leaf(p, path) for path in LEAVES], allow_unused=True)
    grads = {path: (np.zeros(tuple(leaf(p, path).shape)) if g is None else g.detach().numpy()) for path, g in zip(LEAVES, gs)}
    return l.detach().numpy(), z.detach().numpy(), grads


def forward(seeds, p_np, dim, nbridges, lfsteps, target):
    """Losses and end points without building the second-order graph."""
    p = to_torch(p_np, requires_grad=False)
    with torch.enable_grad():
        l, z = losses(seeds, p, dim, nbridges, lfsteps, target, create_graph=False)
    return l.detach().numpy(), z.detach().numpy()


def make_params(dim, nbridges, lfsteps, eps, eta=0.6, seed=0, trainable=("eta", "eps", "vd", "mgridref_y", "md"), device="cpu",
                mean_scale=1.0, sigma=1.0, vd=None):
    """A parameter set with every leaf non-trivial: random mean and md, per-dimension logdiag, eta around 0.6, a non-uniform
    mgridref_y; `vd = (mean, sigma)` replaces the random q by a given one.  -> (params_flat, unflatten, params_fixed) of cmcd_amd.hais.initialize."""
    from cmcd_amd import hais
    rng = np.random.default_rng(seed)
    f32 = lambda a: torch.tensor(np.asarray(a, np.float32))
    drawn = {"mean": f32(mean_scale * rng.standard_normal(dim)), "logdiag": f32(math.log(sigma) + 0.2 * rng.standard_normal(dim))}
    if vd is not None:
        vd = {"mean": f32(vd[0]), "logdiag": f32(np.log(np.asarray(vd[1], np.float64)))}
    md = f32(0.3 * rng.standard_normal(dim))
    ngrid = min(nbridges, 32)
    my = f32(0.5 + rng.random(ngrid + 1))
    return hais.initialize(dim, vdparams=vd if vd is not None else drawn, nbridges=nbridges, lfsteps=lfsteps, eps=eps, eta=eta, mdparams=md, mgridref_y=my,
                           trainable=trainable, device=device)
