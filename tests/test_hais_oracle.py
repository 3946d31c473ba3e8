"""Pins tests/hais_restatement.py (the float64 yardstick of cmcd_hais_bound_grad and cmcd_amd.hais) without a device: the
leap-frog is reversible, one step equals its longhand form, eps = 0 is the mean-field bound, the estimate of Z is unbiased on
a normalised target, and autograd agrees with central differences on every leaf, on and off the grid's nodes.  It also asserts,
on the float64 restatement, that the cases of tests/test_gpu_hais.py are what they are there for: bridges off the grid's
nodes, the four kinds of particle of the floor case (gated_cases.HAIS_FLOOR), and what float32 arithmetic alone costs on the
cases that amplify rounding."""
import math

import numpy as np
import pytest
import torch

import gated_cases as gc
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
    _central_differences(4, 2, None)


def test_autograd_agrees_with_central_differences_off_the_grid_nodes():
    """The same with K = 5 bridges on a grid of ngrid = 3 (four cells): every bridge interpolates (fractions 2/3, 1/3, 0, 2/3,
    1/3 ... asserted), so autograd's mgridref_y gradient is itself pinned where the GPU cases of OFF_GRID use it."""
    frac, _ = hr.fractions(5, 3)
    assert ((frac > 0.05) & (frac < 0.95)).sum() >= 3
    _central_differences(5, 2, 3)


def _central_differences(K, L, ngrid):
    dim = 2
    p_np, _ = _params(dim, K, L, 0.08, seed=1, sigma=2.0, ngrid=ngrid)
    assert p_np["mgridref_y"].shape == ((min(K, 32) if ngrid is None else ngrid) + 1,)
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


# ------------------------------------------------------------------------------------------ the cases of tests/test_gpu_hais.py
@pytest.mark.parametrize("K,ngrid,what", [(40, None, "one-and-two"), (8, 3, "several"), (5, 32, "mostly-empty"), (5, 3, "several")])
def test_off_grid_cases_interpolate(K, ngrid, what):
    """make_params(ngrid=) gives mgridref_y ngrid + 1 entries whatever K; the bridges then sit off the nodes: at least one
    fraction inside (0.05, 0.95), and the cells are filled as the case's comment says.  The fractions are those of np.interp
    on the float32 grids the library reads, and ot.betas_from_grid's betas are np.interp's."""
    flat, un, fixed = hr.make_params(2, K, 1, 0.05, seed=K + 10, ngrid=ngrid)
    p = hr.params_numpy(un, flat)
    G = 32 if ngrid is None else ngrid
    assert p["mgridref_y"].shape == (G + 1,) and p["gridref_x"].shape == (G + 2,) and p["target_x"].shape == (K,)
    assert len(set(np.round(p["mgridref_y"], 6))) == G + 1         # non-uniform
    frac, cell = hr.fractions(K, G)
    inside = (frac > 0.05) & (frac < 0.95)
    assert inside.any(), frac
    # the library's own grids (float32) give the same cells and, within float32, the same fractions
    gx, tx = p["gridref_x"], p["target_x"]
    j = np.clip(np.searchsorted(gx, tx, side="right"), 1, G + 1)
    lib_frac = (tx - gx[j - 1]) / (gx[j] - gx[j - 1])
    ok = np.abs(lib_frac - frac) < 1e-5
    wrapped = np.abs(lib_frac - frac - np.where(j > cell, -1.0, 1.0)) < 1e-5   # a bridge on a node may fall in either cell
    assert (ok | ((j != cell) & wrapped)).all(), (lib_frac, frac)
    assert (j == cell)[inside].all()
    gy = np.concatenate([[0.0], np.cumsum(p["mgridref_y"]) / p["mgridref_y"].sum()])
    betas = ot.betas_from_grid(torch.tensor(p["mgridref_y"]), K).numpy()
    assert np.abs(betas - np.interp(tx, gx, gy)).max() <= 1e-6
    per_cell = np.bincount(cell, minlength=G + 2)[1:]
    if what == "one-and-two":
        assert (per_cell == 1).any() and (per_cell == 2).any() and inside.sum() >= 3 * K // 4
    elif what == "several":
        assert (per_cell >= 2).sum() >= 1 and inside.sum() >= 3
    else:
        assert (per_cell == 0).sum() >= 28 and inside.sum() >= 3


def test_trace_records_every_evaluation():
    """K L + 1 entries, the first at z_0 and the last at z_K, log p unfloored; the float32 switch returns float32 and agrees."""
    K, L = 3, 2
    flat, un, fixed = hr.make_params(2, K, L, 0.1, seed=2, sigma=15.0, mean_scale=5.0)
    p_np = hr.params_numpy(un, flat)
    seeds = np.arange(1, 10, dtype=np.int32)
    trace = {}
    l, z = hr.forward(seeds, p_np, 2, K, L, "many_gmm", trace=trace)
    assert len(trace["lp"]) == K * L + 1 == len(trace["z"])
    assert np.array_equal(trace["z"][-1], z)
    e0, _, _ = prng.particle_noise_uha(seeds, 2, K)
    z0 = hr.z0_of(hr.to_torch(p_np, requires_grad=False), torch.tensor(e0.astype(np.float64))).numpy()
    assert np.array_equal(trace["z"][0], z0)
    for lp, zz in zip(trace["lp"], trace["z"]):
        assert np.array_equal(lp, ot.logp_many_gmm_unfloored(torch.tensor(zz)).numpy())
    l2, z2 = hr.forward(seeds, p_np, 2, K, L, "many_gmm")
    assert np.array_equal(l, l2) and np.array_equal(z, z2)          # tracing changes nothing
    l32, z32 = hr.forward(seeds, p_np, 2, K, L, "many_gmm", dtype=torch.float32)
    assert l32.dtype == np.float32 and z32.dtype == np.float32
    assert np.abs(l32 - l).max() <= 1e-3 * np.abs(l).max() and 0 < np.abs(z32 - z).max() <= 1e-3


def _floor_case():
    seeds, cat = gc.hais_floor_batch()
    flat, un, fixed = gc.hais_floor_params()
    c = gc.HAIS_FLOOR
    return seeds, cat, hr.params_numpy(un, flat), (c["dim"], c["K"], c["L"])


def test_floor_case_pool_and_batch():
    """gated_cases.HAIS_FLOOR on the seeds 1 .. 2048: the guard band drops 8 (at most 2 %), the band-clear seeds fall into
    118 / 6 / 1361 / 555 of the four categories, the ridge guard drops 339 more, and the batch is 16 / 4 / 5 / 8."""
    seeds, near, ridge, cat = gc.hais_floor_pool()
    print("band", int(near.sum()), "ridge", int((ridge & ~near).sum()),
          {name: (int(((cat == k) & ~near).sum()), int(((cat == k) & ~near & ~ridge).sum())) for k, name in enumerate(gc.HAIS_FLOOR_CATEGORIES)})
    assert near.mean() <= 0.02
    assert int(near.sum()) == 8 and [int(((cat == k) & ~near).sum()) for k in range(4)] == [118, 6, 1361, 555]
    assert not ridge[cat == 2].any()                               # no unfloored evaluation, no ridge
    b_seeds, b_cat = gc.hais_floor_batch()
    assert len(b_seeds) == 33 and (np.diff(b_seeds) > 0).all()
    counts = [int((b_cat == k).sum()) for k in range(4)]
    assert counts == list(gc.HAIS_FLOOR["take"])
    assert counts[0] >= 8 and counts[1] >= 2 and counts[2] >= 2 and counts[3] >= 4
    # the categories again, from the batch's own chain
    _, _, p_np, (dim, K, L) = _floor_case()
    trace = {}
    l, _ = hr.forward(b_seeds, p_np, dim, K, L, "many_gmm", trace=trace)
    lp = np.stack(trace["lp"])
    fl = lp <= gc.FLOOR
    assert (np.abs(lp - gc.FLOOR) > gc.DELTA * -gc.FLOOR).all()
    assert np.array_equal(fl[:-1].any(0) & ~fl[-1], b_cat == 0)
    assert np.array_equal(fl[-1] & ~fl.all(0), b_cat == 1)
    assert np.array_equal(fl.all(0), b_cat == 2)
    assert np.array_equal(~fl.any(0), b_cat == 3)
    assert np.array_equal(np.isposinf(l), fl[-1]) and int(fl[-1].sum()) == 9
    assert (gc.component_gap(np.stack(trace["z"]))[~fl] >= gc.RIDGE_NATS).all()


def test_floor_case_gradient_is_finite_and_the_gate_moves_it():
    """Nine losses are +inf and every leaf's gradient is finite and non-zero; on the finite-loss particles the unfloored
    target's gradient differs on some leaf by more than SEPARATION = 10 x 2e-3 of the leaf's scale (measured: every leaf but
    eta by 50 % or more, eta by 9 %)."""
    seeds, cat, p_np, (dim, K, L) = _floor_case()
    l, _, g = hr.bound_and_grad(seeds, p_np, dim, K, L, "many_gmm")
    assert int(np.isposinf(l).sum()) == 9 and not np.isnan(l).any()
    for path in hr.LEAVES:
        assert np.isfinite(g[path]).all() and np.abs(g[path]).max() > 0, path
    fin = np.isfinite(l)
    g_true = hr.bound_and_grad(seeds[fin], p_np, dim, K, L, "many_gmm")[2]
    g_open = hr.bound_and_grad(seeds[fin], p_np, dim, K, L, ot.logp_many_gmm_unfloored)[2]
    sep = {path: float(np.abs(g_open[path] - g_true[path]).max() / np.abs(g_true[path]).max()) for path in hr.LEAVES}
    print(sep)
    assert max(sep.values()) > gc.SEPARATION
    assert sum(v > gc.SEPARATION for v in sep.values()) == len(hr.LEAVES)


def test_float32_alone_stays_a_tenth_of_the_bar_on_the_amplifying_cases():
    """The restatement in float32 against float64, leaf by leaf, on the floor case and on eta = 0.99 (gmm, n = 37, K = 4,
    L = 2 as tests/test_gpu_hais.py builds it): at or below 2e-4, a tenth of the GPU comparison's bar.  Measured: floor case
    2.0e-7 (mgridref_y), eta = 0.99 4.4e-7 (eps), eta = 0 5.5e-7 (eta)."""
    seeds, cat, p_np, (dim, K, L) = _floor_case()
    gap = hr.float32_gap(seeds, p_np, dim, K, L, "many_gmm")
    print("floor", gap)
    assert max(gap.values()) <= gc.BAR / 10
    for eta in (0.0, 0.99):
        flat, un, fixed = hr.make_params(2, 4, 2, 0.05, eta=eta, seed=4 + 10 * 2, mean_scale=1.0, sigma=2.0)
        gap = hr.float32_gap(np.arange(1, 38, dtype=np.int32), hr.params_numpy(un, flat), 2, 4, 2, "gmm")
        print("eta", eta, gap)
        assert max(gap.values()) <= gc.BAR / 10
