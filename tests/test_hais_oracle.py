"""Pins tests/hais_restatement.py (the float64 yardstick of cmcd_hais_bound_grad and cmcd_amd.hais) without a device: the
leap-frog is reversible, one step equals its longhand form, eps = 0 is the mean-field bound, the estimate of Z is unbiased on
a normalised target, and autograd agrees with central differences on every leaf."""
import math

import numpy as np
import pytest
import torch

import hais_restatement as hr
from oracle import cmcd_oracle_torch as ot
from oracle import prng


def _params(dim, K, L, eps, **kw):
    flat, un, fixed = hr.make_params(dim, K, L, eps, **kw)
    return hr.params_numpy(un, flat), fixed


@pytest.mark.parametrize("target,dim", [("gmm", 2), ("funnel", 10)])
@pytest.mark.parametrize("L", [1, 3])
def test_leapfrog_is_reversible(target, dim, L):
    """Negate r and run the bridge's leap-frog again: back at (z, -rho)."""
    p_np, _ = _params(dim, 4, L, 0.05, seed=3)
    p = hr.to_torch(p_np, requires_grad=False)
    rng = np.random.default_rng(5)
    z = torch.tensor(rng.standard_normal((16, dim)))
    rho = torch.tensor(rng.standard_normal((16, dim)))
    logp = ot.TARGETS[target]
    z1, r1 = hr.leapfrog(p, logp, z, rho, 0.4, L, create_graph=False)
    assert float((z1 - z).abs().max()) > 1e-3                     # it moved
    z2, r2 = hr.leapfrog(p, logp, z1.detach(), -r1.detach(), 0.4, L, create_graph=False)
    assert float((z2 - z).abs().max()) <= 1e-10
    assert float((r2 + rho).abs().max()) <= 1e-10


@pytest.mark.parametrize("target,dim", [("gmm", 2), ("funnel", 10)])
def test_single_step_equals_the_longhand_form(target, dim):
    """K = 1, L = 1, eta = 0, md = 0:  z' = z0 + eps (xi - eps/2 gU(z0)),  r = xi - eps/2 (gU(z0) + gU(z')),
    loss = log q(z0) + |r|^2 / 2 - |xi|^2 / 2 - log p(z')."""
    flat, un, fixed = hr.make_params(dim, 1, 1, 0.07, eta=0.0, seed=2)
    p_np = hr.params_numpy(un, flat)
    p_np["md"] = np.zeros(dim)
    seeds = np.arange(1, 12, dtype=np.int32)
    got, z_got = hr.forward(seeds, p_np, dim, 1, 1, target)

    p = hr.to_torch(p_np, requires_grad=False)
    logp = ot.TARGETS[target]
    e0, _, xi = prng.particle_noise_uha(seeds, dim, 1)
    xi = torch.tensor(xi[:, 0, :].astype(np.float64))
    z0 = hr.z0_of(p, torch.tensor(e0.astype(np.float64)))
    m = p["mgridref_y"]
    assert m.shape[0] == 2
    beta = m[0] / (m[0] + m[1])            # interp of [0, m0 / S, 1] on [0, 1/2, 1] at 1/2
    eps = p["eps"]
    g0 = hr.grad_u(p, logp, z0, beta, create_graph=False)
    z1 = z0 + eps * (xi - eps / 2 * g0)
    g1 = hr.grad_u(p, logp, z1, beta, create_graph=False)
    r = xi - eps / 2 * (g0 + g1)
    want = hr.log_q(p["vd"], z0) + (r ** 2).sum(-1) / 2 - (xi ** 2).sum(-1) / 2 - logp(z1)
    assert np.abs(got - want.numpy()).max() <= 1e-12
    assert np.abs(z_got - z1.numpy()).max() <= 1e-12


@pytest.mark.parametrize("target,dim", [("gmm", 2), ("funnel", 10), ("many_gmm", 2)])
def test_zero_step_size_is_the_mean_field_bound(target, dim):
    p_np, _ = _params(dim, 4, 2, 0.0, seed=4, sigma=3.0)
    seeds = np.arange(1, 33, dtype=np.int32)
    got, z = hr.forward(seeds, p_np, dim, 4, 2, target)
    p = hr.to_torch(p_np, requires_grad=False)
    e0, _, _ = prng.particle_noise_uha(seeds, dim, 4)
    z0 = hr.z0_of(p, torch.tensor(e0.astype(np.float64)))
    want = (hr.log_q(p["vd"], z0) - ot.TARGETS[target](z0)).numpy()
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin)
    assert np.abs(got[fin] - want[fin]).max() <= 1e-12
    assert np.array_equal(z, z0.numpy())


def _unbiased_case():
    from cmcd_amd import hais
    vd = {"mean": torch.tensor([0.7, 0.6]), "logdiag": torch.log(torch.tensor([2.5, 2.25]))}
    flat, un, fixed = hais.initialize(2, vdparams=vd, nbridges=8, lfsteps=2, eps=0.2, eta=0.3, mdparams=torch.tensor([0.1, -0.1]),
                                      mgridref_y=torch.tensor([1.0, 1.2, 0.8, 1.0, 1.1, 0.9, 1.0, 1.3, 0.7]), device="cpu")
    return hr.params_numpy(un, flat)


def test_estimate_of_z_is_unbiased_on_the_normalised_gmm():
    """gmm is normalised: mean exp(-loss) = 1 within 4 standard errors (K = 8, 4096 seeds), on a parameter set whose
    importance weights are healthy (ESS above a quarter of the seeds: a condition of the check, asserted)."""
    seeds = np.arange(1, 4097, dtype=np.int32)
    l, _ = hr.forward(seeds, _unbiased_case(), 2, 8, 2, "gmm")
    assert np.isfinite(l).all()
    w = np.exp(-l)
    ess = w.sum() ** 2 / (w ** 2).sum()
    assert ess > len(seeds) / 4, ess
    se = w.std(ddof=1) / math.sqrt(len(w))
    assert abs(w.mean() - 1.0) <= 4 * se, (w.mean(), se)


def test_autograd_agrees_with_central_differences_on_every_leaf():
    """float64, step 1e-6, the sum over 8 seeds on gmm with K = 4, L = 2: within 1e-5 of the leaf's largest entry."""
    dim, K, L = 2, 4, 2
    p_np, _ = _params(dim, K, L, 0.08, seed=1, sigma=2.0)
    seeds = np.arange(1, 9, dtype=np.int32)
    p = hr.to_torch(p_np)
    l, _ = hr.losses(seeds, p, dim, K, L, "gmm")
    leaves = [hr.leaf(p, path) for path in hr.LEAVES]
    grads = torch.autograd.grad(l.sum(), leaves)

    def total(q):
        return float(hr.forward(seeds, q, dim, K, L, "gmm")[0].sum())

    h = 1e-6
    for path, g in zip(hr.LEAVES, grads):
        g = g.detach().numpy().reshape(-1)
        assert np.abs(g).max() > 0, path
        fd = np.zeros_like(g)
        for k in range(g.size):
            vals = []
            for sgn in (+1, -1):
                q = {kk: (dict(vv) if isinstance(vv, dict) else vv) for kk, vv in p_np.items()}
                node = q
                for key in path[:-1]:
                    node = node[key]
                a = np.array(node[path[-1]], np.float64).reshape(-1).copy()
                a[k] += sgn * h
                node[path[-1]] = a.reshape(np.shape(p_np[path[0]] if len(path) == 1 else p_np[path[0]][path[1]]))
                vals.append(total(q))
            fd[k] = (vals[0] - vals[1]) / (2 * h)
        assert np.abs(fd - g).max() <= 1e-5 * np.abs(g).max(), (path, fd, g)
