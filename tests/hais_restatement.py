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


def to_torch(p, requires_grad=True, dtype=torch.float64):
    """torch leaves (float64 unless `dtype` says otherwise) of the six differentiable leaves (the two grids are not needed:
    both are uniform)."""
    t = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=dtype).requires_grad_(requires_grad)
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


def leapfrog(p, logp_fn, z, rho, beta, lfsteps, create_graph=True, record=None):
    """ais_utils.py:26-57 without delta_H; grad K(rho) = rho / s^2.  `record(z)` is called at the position of the opening kick
    and of every inner kick (the closing kick's position is the next bridge's opening one, or z_K)."""
    eps, iv = p["eps"], torch.exp(-2.0 * p["md"])
    if record is not None:
        record(z)
    rho = rho - eps * grad_u(p, logp_fn, z, beta, create_graph) / 2.0
    z = z + eps * rho * iv
    for _ in range(lfsteps - 1):
        if record is not None:
            record(z)
        rho = rho - eps * grad_u(p, logp_fn, z, beta, create_graph)
        z = z + eps * rho * iv
    rho = rho - eps * grad_u(p, logp_fn, z, beta, create_graph) / 2.0
    return z, rho


def noise(seeds, dim, nbridges, dtype=torch.float64):
    e0, n0, xi = prng.particle_noise_uha(np.asarray(seeds), dim, nbridges)
    t = lambda a: torch.tensor(a.astype(np.float64), dtype=dtype)
    return t(e0), t(n0), t(xi)


def z0_of(p, e0):
    return torch.exp(p["vd"]["logdiag"]) * e0 + p["vd"]["mean"]


def losses(seeds, p, dim, nbridges, lfsteps, target, create_graph=True, trace=None):
    """-> (losses[N], z[N, dim]) in the dtype of `p` (a to_torch dict: float64 unless asked otherwise), differentiable in its
    leaves.  `trace` (a dict) receives, at each of the K L + 1 evaluations in chain order, log p BEFORE its floor under "lp"
    ([N] NumPy arrays) and the position under "z" ([N, dim]): the last entries are the end point's."""
    logp_fn = ot.TARGETS[target] if isinstance(target, str) else target
    record = None
    if trace is not None:
        raw = getattr(logp_fn, "unfloored", logp_fn)

        def record(zz):
            with torch.no_grad():
                trace.setdefault("lp", []).append(raw(zz.detach()).numpy().copy())
                trace.setdefault("z", []).append(zz.detach().numpy().copy())
    e0, n0, xi = noise(seeds, dim, nbridges, dtype=p["eps"].dtype)
    s = torch.exp(p["md"])
    z = z0_of(p, e0)
    w = -log_q(p["vd"], z)
    if nbridges >= 1:
        betas = ot.betas_from_grid(p["mgridref_y"], nbridges)
        rho_prev = s * n0
        for i in range(nbridges):
            rho = p["eta"] * rho_prev + torch.sqrt(1.0 - p["eta"] ** 2) * s * xi[:, i, :]
            z, r = leapfrog(p, logp_fn, z, rho, betas[i], lfsteps, create_graph, record)
            w = w + log_mom(p["md"], r) - log_mom(p["md"], rho)
            rho_prev = r
    if record is not None:
        record(z)
    w = w + logp_fn(z)
    return -w, z


def bound_and_grad(seeds, p_np, dim, nbridges, lfsteps, target, dtype=torch.float64):
    """-> (losses, z, {leaf path: d mean(losses) / d leaf}) as NumPy; what jax.grad(bm.compute_bound, 1) returns, leaf by leaf.
    `dtype = torch.float32` runs the same arithmetic in single precision: only to measure what float32 alone costs on a case."""
    p = to_torch(p_np, dtype=dtype)
    l, z = losses(seeds, p, dim, nbridges, lfsteps, target)
    gs = torch.autograd.grad(l.mean(), [leaf(p, path) for path in LEAVES], allow_unused=True)
    grads = {path: (np.zeros(tuple(leaf(p, path).shape)) if g is None else g.detach().numpy().astype(np.float64))
             for path, g in zip(LEAVES, gs)}
    return l.detach().numpy(), z.detach().numpy(), grads


def forward(seeds, p_np, dim, nbridges, lfsteps, target, trace=None, dtype=torch.float64):
    """Losses and end points without building the second-order graph."""
    p = to_torch(p_np, requires_grad=False, dtype=dtype)
    with torch.enable_grad():
        l, z = losses(seeds, p, dim, nbridges, lfsteps, target, create_graph=False, trace=trace)
    return l.detach().numpy(), z.detach().numpy()


def float32_gap(seeds, p_np, dim, nbridges, lfsteps, target):
    """{leaf path: max |g32 - g64| / max |g64|}: the restatement's gradient in float32 against its float64 run, same seeds."""
    g64 = bound_and_grad(seeds, p_np, dim, nbridges, lfsteps, target)[2]
    g32 = bound_and_grad(seeds, p_np, dim, nbridges, lfsteps, target, dtype=torch.float32)[2]
    return {path: float(np.abs(g32[path] - g64[path]).max() / np.abs(g64[path]).max()) for path in LEAVES}


def fractions(nbridges, ngrid):
    """The interpolation weight of every bridge inside its cell of gridref_x (ot.betas_from_grid's `frac`), float64."""
    pos = np.arange(1, nbridges + 1, dtype=np.float64) / (nbridges + 1) * (ngrid + 1)
    j = np.clip(np.floor(pos).astype(np.int64) + 1, 1, ngrid + 1)
    return pos - (j - 1), j


def make_params(dim, nbridges, lfsteps, eps, eta=0.6, seed=0, trainable=("eta", "eps", "vd", "mgridref_y", "md"), device="cpu",
                mean_scale=1.0, sigma=1.0, vd=None, ngrid=None, mean_add=None):
    """A parameter set with every leaf non-trivial: random mean and md, per-dimension logdiag, eta around 0.6, a non-uniform
    mgridref_y of length `ngrid + 1` (default min(nbridges, 32), the reference's; any other value takes the bridges off the
    grid's nodes); `vd = (mean, sigma)` replaces the random q by a given one, `mean_add` shifts the drawn mean.
    -> (params_flat, unflatten, params_fixed) of cmcd_amd.hais.initialize."""
    from cmcd_amd import hais
    rng = np.random.default_rng(seed)
    f32 = lambda a: torch.tensor(np.asarray(a, np.float32))
    drawn = {"mean": f32(mean_scale * rng.standard_normal(dim)), "logdiag": f32(math.log(sigma) + 0.2 * rng.standard_normal(dim))}
    if vd is not None:
        vd = {"mean": f32(vd[0]), "logdiag": f32(np.log(np.asarray(vd[1], np.float64)))}
    if mean_add is not None:
        drawn["mean"] = drawn["mean"] + f32(mean_add)
    md = f32(0.3 * rng.standard_normal(dim))
    if ngrid is None:
        ngrid = min(nbridges, 32)
    my = f32(0.5 + rng.random(ngrid + 1))
    return hais.initialize(dim, vdparams=vd if vd is not None else drawn, nbridges=nbridges, lfsteps=lfsteps, eps=eps, eta=eta, mdparams=md, mgridref_y=my,
                           trainable=trainable, device=device)
