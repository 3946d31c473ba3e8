"""UHA (Hamiltonian AIS) on the GPU — cmcd_amd.hais over cmcd_hais_bound_grad (cmcd_amd/csrc/cmcd_hais.hip) — against the float64
restatement of tests/hais_restatement.py, which tests/test_hais_oracle.py pins on the CPU: forward parity under the project's
bar (tests/helpers.compare_losses, check_stats), gradient parity against autograd under the rule of tests/test_gpu_grad.py,
bit-reproducibility, capture, error paths, training and the command-line driver.

Parameter sets have every leaf non-trivial (hais_restatement.make_params: random mean and md, per-dimension logdiag, eta 0.6,
non-uniform mgridref_y); eps per target so that the restatement's losses are finite on every seed — except the many_gmm floor
cases, whose q is wide enough (forward) or far enough out (gated_cases.HAIS_FLOOR, gradient) for log p to be floored to -inf.

Which gradient case reaches what in cmcd_hais.hip: n = 145 / 133 (10 / 9 tiles) run hais_grad_kernel in three workgroups, the
last with two (three) idle waves, and the eight-wide loop of hais_reduce_kernel once plus its remainder loop; K = 40, (K, ngrid)
= (8, 3) and (5, 32) put the bridges off the grid's nodes (frac inside (0, 1), cells with several bridges and with none);
the floor case runs the lp > -1e4 gate of eval_hess; n_mixes = 17 the generic component loops behind tile_stage_many_gmm;
n_total the omega of the C call."""
import functools
import math
import types

import numpy as np
import pytest
import torch

import gated_cases as gc
import hais_restatement as hr
from cmcd_amd import boundingmachine as bm
from cmcd_amd import hais, model_handler, opt
from helpers import check_stats, compare_losses

pytestmark = pytest.mark.gpu

# (dim, eps, q's sigma, scale of q's mean): step sizes well inside the leap-frog's stability range of each target
TARGETS = {"gmm": (2, 0.05, 2.0, 1.0), "funnel": (10, 0.05, 1.0, 0.5), "many_gmm": (2, 0.1, 15.0, 5.0)}


@functools.lru_cache(maxsize=None)
def target_of(name):
    return model_handler.load_model(name)[0]


DEVICE = "cuda"


@functools.lru_cache(maxsize=None)
def built(name, K, L, trainable=("eta", "eps", "vd", "mgridref_y", "md"), eps=None, sigma=None, ngrid=None, eta=0.6):
    dim, eps0, sigma0, mean_scale = TARGETS[name]
    flat, un, fixed = hr.make_params(dim, K, L, eps0 if eps is None else eps, seed=K + 10 * L, trainable=trainable,
                                     device=DEVICE, mean_scale=mean_scale, sigma=sigma0 if sigma is None else sigma,
                                     ngrid=ngrid, eta=eta)
    return flat, un, fixed, hr.params_numpy(un, flat)


@functools.lru_cache(maxsize=None)
def many_gmm_of(n_mixes):
    """(the library's target, the restatement's log p) of many_gmm with `n_mixes` components."""
    from oracle import cmcd_oracle_torch as ot
    tgt = model_handler.load_model("many_gmm", types.SimpleNamespace(n_mixes=n_mixes))[0]
    assert tgt.n_mixes == n_mixes and tgt.consts_on("cpu").numel() == 1 + 2 * n_mixes
    return tgt, functools.partial(ot.logp_many_gmm, n_mixes=n_mixes)


@functools.lru_cache(maxsize=None)
def reference(name, K, L, n, with_grad=False, n_mixes=None, **kw):
    """The restatement on seeds 1 .. n, computed once per case and shared (read-only)."""
    _, _, fixed, p_np = built(name, K, L, **kw)
    seeds = np.arange(1, n + 1, dtype=np.int32)
    logp = name if n_mixes is None else many_gmm_of(n_mixes)[1]
    if with_grad:
        return hr.bound_and_grad(seeds, p_np, fixed[0], K, L, logp)
    return hr.forward(seeds, p_np, fixed[0], K, L, logp) + (None,)


def dev(seeds):
    return torch.from_numpy(np.asarray(seeds, np.int32)).cuda()


def run_forward(name, K, L, seeds, **kw):
    flat, un, fixed, _ = built(name, K, L, **kw)
    losses, z, stats = hais.bound_forward(dev(seeds), flat, un, fixed, target_of(name))
    torch.cuda.synchronize()
    return losses, z, stats


# ------------------------------------------------------------------------------------------ forward parity
FORWARD = [("gmm", n, K, L) for n in (1, 16, 37) for K in (1, 8) for L in (1, 3)] + [
    ("funnel", 37, 8, 2),
    ("gmm", 37, 64, 1),          # the long-chain branch of compare_losses
    ("gmm", 1040, 8, 1),         # 65 tiles: the finalize launch merges more than one round of records
    ("many_gmm", 37, 8, 1), ("many_gmm", 37, 8, 3), ("many_gmm", 145, 4, 2),
    ("funnel", 5, 2, 1), ("funnel", 133, 2, 2),
]


@pytest.mark.parametrize("name,n,K,L", FORWARD)
def test_forward_matches_the_restatement(hip_lib, name, n, K, L):
    l_ref, z_ref, _ = reference(name, K, L, n)
    assert np.isfinite(l_ref).all(), "eps is chosen so that every loss of the restatement is finite"
    losses, z, stats = run_forward(name, K, L, np.arange(1, n + 1))
    rep = compare_losses(losses.cpu().numpy(), l_ref, z.cpu().numpy(), z_ref, tag=f"{name} n={n} K={K} L={L}", K=K)
    print(rep, check_stats(stats, losses, tag=name))
    mean, (l2, z2) = hais.compute_bound(dev(np.arange(1, n + 1)), *built(name, K, L)[:3], target_of(name))
    assert torch.equal(l2, losses) and torch.equal(z2, z)
    assert abs(float(mean) - float(losses.double().mean())) <= 1e-5 * max(1.0, abs(float(mean)))


@functools.lru_cache(maxsize=None)
def floor_case():
    """many_gmm, K = 8, L = 1 under a q of sigma 40: among the first 4096 seeds, 36 whose end point is far above the floor of
    log p (-1e4) and one far below it.  -> (seeds[37], reference losses, reference z, index of the floored one or None)."""
    _, _, fixed, p_np = built("many_gmm", 8, 1, sigma=40.0)
    from oracle import cmcd_oracle_torch as ot
    all_seeds = np.arange(1, 4097, dtype=np.int32)
    l, z = hr.forward(all_seeds, p_np, 2, 8, 1, "many_gmm")
    raw = ot.logp_many_gmm_unfloored(torch.tensor(z)).numpy()
    clear = np.flatnonzero(raw > -5e3)[:36]
    deep = np.flatnonzero(raw < -1.5e4)[:1]
    pick = np.sort(np.concatenate([clear, deep]))
    return all_seeds[pick], l[pick], z[pick], (int(np.flatnonzero(pick == deep[0])[0]) if len(deep) else None)


def test_forward_many_gmm_with_a_floored_end_point(hip_lib):
    seeds, l_ref, z_ref, floored = floor_case()
    assert floored is not None, "no end point below the floor among the first 4096 seeds: widen q"
    assert len(seeds) == 37 and np.isinf(l_ref[floored]) and np.isfinite(np.delete(l_ref, floored)).all()
    losses, z, stats = run_forward("many_gmm", 8, 1, seeds, sigma=40.0)
    assert losses[floored].item() == math.inf
    rep = compare_losses(losses.cpu().numpy(), l_ref, z.cpu().numpy(), z_ref, tag="many_gmm floor", K=8)
    print(rep, check_stats(stats, losses, tag="many_gmm floor"))


@pytest.mark.parametrize("n_mixes", [7, 17, 64])
def test_forward_many_gmm_with_other_mixture_sizes(hip_lib, n_mixes):
    """config.n_mixes != 40 takes the generic component loops of pass1 / pass2 behind tile_stage_many_gmm (64: the library's
    maximum), as tests/test_gpu_parity.py::test_many_gmm_with_other_mixture_sizes does for the older modes."""
    n, K, L = 37, 4, 2
    l_ref, z_ref, _ = reference("many_gmm", K, L, n, n_mixes=n_mixes)
    assert np.isfinite(l_ref).all()
    flat, un, fixed, _ = built("many_gmm", K, L)
    losses, z, stats = hais.bound_forward(dev(np.arange(1, n + 1)), flat, un, fixed, many_gmm_of(n_mixes)[0])
    torch.cuda.synchronize()
    rep = compare_losses(losses.cpu().numpy(), l_ref, z.cpu().numpy(), z_ref, tag=f"many_gmm n_mixes={n_mixes}", K=K)
    print(rep, check_stats(stats, losses, tag=f"n_mixes={n_mixes}"))
    l40, _, _ = run_forward("many_gmm", K, L, np.arange(1, n + 1))
    assert not torch.equal(l40, losses)                            # it is another target


# ------------------------------------------------------------------------------------------ gradient parity
def compare_grad(tag, un, g, ref_by_leaf, tol=2e-3):
    """The rule of tests/test_gpu_grad.py:_compare: per leaf max abs error / max |ref| <= 2e-3, exact zeros where the
    reference is zero, cosine over the whole vector > 1 - 1e-5."""
    g = g.double().cpu()
    g_ref = torch.zeros_like(g)
    for path, val in ref_by_leaf.items():
        off, shape = next((o, s) for p, (o, s) in un.layout.items() if p[1:] == path)
        g_ref[off:off + max(1, int(np.prod(shape)))] = torch.as_tensor(np.asarray(val, np.float64)).reshape(-1)
    worst = {}
    for path, (off, shape) in un.layout.items():
        numel = max(1, int(np.prod(shape)))
        a, r = g[off:off + numel], g_ref[off:off + numel]
        scale = max(float(r.abs().max()), 1e-12)
        worst["/".join(map(str, path))] = (float((a - r).abs().max()) / scale, scale)
        if float(r.abs().max()) == 0.0:
            assert float(a.abs().max()) == 0.0, f"{path}: expected exactly zero gradient"
    bad = {k: v for k, v in worst.items() if v[0] > tol and v[1] > 1e-9}
    print(tag, {k: "%.1e" % v[0] for k, v in worst.items()})
    assert not bad, f"gradient mismatch (max abs err / max |ref|, max |ref|): {bad}"
    cos = float((g * g_ref).sum() / (g.norm() * g_ref.norm()))
    assert cos > 1 - 1e-5, cos
    return g_ref


GRAD = [("gmm", 37, 8, 1), ("gmm", 37, 8, 3), ("funnel", 37, 8, 2), ("many_gmm", 37, 8, 1),
        ("gmm", 1, 1, 1),            # one particle, one bridge
        ("gmm", 17, 1, 3),           # one bridge with inner leap-frog steps; the second tile holds one particle
        ("gmm", 16, 8, 1),           # a full tile
        ("funnel", 5, 2, 1), ("funnel", 21, 3, 3),
        # 10 tiles: three workgroups of the sweep, the last with two idle waves; the reduction's eight-wide loop runs once
        # and its remainder loop twice; the last tile holds one particle
        ("gmm", 145, 4, 2), ("many_gmm", 145, 4, 1),
        ("funnel", 133, 2, 2)]       # 9 tiles, the last with five particles


@pytest.mark.parametrize("name,n,K,L", GRAD)
def test_gradient_matches_autograd(hip_lib, name, n, K, L):
    l_ref, z_ref, g_ref = reference(name, K, L, n, with_grad=True)
    assert np.isfinite(l_ref).all(), "no particle at the floor: the gradient check needs finite losses"
    flat, un, fixed, _ = built(name, K, L)
    grad, (losses, z) = hais.grad_and_loss(dev(np.arange(1, n + 1)), flat, un, fixed, target_of(name))
    torch.cuda.synchronize()
    np.testing.assert_allclose(losses.cpu().numpy(), l_ref, rtol=2e-3, atol=2e-3)
    for path in hr.LEAVES:
        assert np.abs(g_ref[path]).max() > 0, f"{path}: the reference gradient of a trainable leaf is zero"
    compare_grad(f"{name} n={n} K={K} L={L}", un, grad, g_ref)


def _gradient_case(tag, name, n, K, L, **kw):
    l_ref, z_ref, g_ref = reference(name, K, L, n, with_grad=True, **kw)
    assert np.isfinite(l_ref).all(), "no particle at the floor: the gradient check needs finite losses"
    flat, un, fixed, _ = built(name, K, L, **kw)
    grad, (losses, z) = hais.grad_and_loss(dev(np.arange(1, n + 1)), flat, un, fixed, target_of(name))
    torch.cuda.synchronize()
    compare_losses(losses.cpu().numpy(), l_ref, z.cpu().numpy(), z_ref, tag=tag, K=K)
    compare_grad(tag, un, grad, g_ref)
    return g_ref


# (K, ngrid): the bridges' abscissae i / (K + 1) against the grid's nodes j / (ngrid + 1); tests/test_hais_oracle.py asserts
# what each pair is here for
OFF_GRID = [(40, None),     # ngrid = 32, the reference's for K > 32: fractions inside (0, 1), cells with one and with two bridges
            (8, 3),         # two bridges in every cell
            (5, 32)]        # 28 of the 33 cells empty


@pytest.mark.parametrize("K,ngrid", OFF_GRID)
def test_gradient_with_bridges_off_the_grid_nodes(hip_lib, K, ngrid):
    """d beta -> d mgridref_y through a real interpolation (hais_reduce_kernel's gather with frac inside (0, 1))."""
    g_ref = _gradient_case(f"gmm n=37 K={K} ngrid={ngrid}", "gmm", 37, K, 1, ngrid=ngrid)
    m = g_ref[("mgridref_y",)]
    assert m.shape == ((32 if ngrid is None else ngrid) + 1,) and np.abs(m).max() > 0


@pytest.mark.parametrize("eta", [0.0, 0.99])
def test_gradient_at_the_edges_of_eta(hip_lib, eta):
    """eta = 0 (the refresh forgets the momentum; ce = 1) and eta = 0.99, its projection bound, where the sweep's
    ic2 = 1 / (1 - eta^2) is about 50.  float32 alone costs 5.5e-7 / 4.4e-7 of a leaf here (hais_restatement.float32_gap,
    asserted below 2e-4 in tests/test_hais_oracle.py)."""
    _gradient_case(f"gmm n=37 K=4 L=2 eta={eta}", "gmm", 37, 4, 2, eta=eta)


def test_gradient_many_gmm_with_17_components(hip_lib):
    """The generic component loop of eval_hess (n_mixes != 40) through the sweep."""
    n, K, L = 37, 4, 2
    l_ref, z_ref, g_ref = reference("many_gmm", K, L, n, with_grad=True, n_mixes=17)
    assert np.isfinite(l_ref).all()
    flat, un, fixed, _ = built("many_gmm", K, L)
    grad, (losses, z) = hais.grad_and_loss(dev(np.arange(1, n + 1)), flat, un, fixed, many_gmm_of(17)[0])
    torch.cuda.synchronize()
    compare_losses(losses.cpu().numpy(), l_ref, z.cpu().numpy(), z_ref, tag="many_gmm n_mixes=17", K=K)
    for path in hr.LEAVES:
        assert np.abs(g_ref[path]).max() > 0, path
    compare_grad("many_gmm n_mixes=17", un, grad, g_ref)


@functools.lru_cache(maxsize=None)
def floor_sweep_reference():
    seeds, cat = gc.hais_floor_batch()
    flat, un, fixed = gc.hais_floor_params()
    c = gc.HAIS_FLOOR
    return (seeds, cat) + hr.bound_and_grad(seeds, hr.params_numpy(un, flat), c["dim"], c["K"], c["L"], c["target"])


def test_gradient_with_the_floor_acting_in_the_sweep(hip_lib):
    """gated_cases.HAIS_FLOOR: 33 particles of which 16 are floored at early evaluations and inside at z_K, 4 end floored
    (loss +inf, gradient finite), 5 are floored throughout and 8 never; tests/test_hais_oracle.py asserts that on the float64
    restatement, and that opening the gate moves every leaf but eta by 50 % or more (eta: 9 %) against a bar of 0.2 %.  The
    sweep recomputes the gate in Target::eval_hess and undoes kicks with its score; the forward kernel took it from
    Target::eval.  float32 alone costs at most 2.0e-7 of a leaf on this batch (mgridref_y; hais_restatement.float32_gap).
    Run a second time in reverse order, so that floored and unfloored particles sit in other tiles and lanes."""
    seeds, cat, l_ref, z_ref, g_ref = floor_sweep_reference()
    flat, un, fixed = gc.hais_floor_params("cuda")
    tgt = target_of("many_gmm")
    inf = np.isinf(l_ref)
    assert len(seeds) == 33 and int(inf.sum()) == 9 and np.array_equal(inf, (cat == 1) | (cat == 2))
    grad, (losses, z) = hais.grad_and_loss(dev(seeds), flat, un, fixed, tgt)
    torch.cuda.synchronize()
    assert np.array_equal(np.isposinf(losses.cpu().numpy()), inf)
    print(compare_losses(losses.cpu().numpy(), l_ref, z.cpu().numpy(), z_ref, tag="UHA floor", K=4))
    assert bool(torch.isfinite(grad).all())
    compare_grad("UHA floor", un, grad, g_ref)
    perm = np.arange(len(seeds))[::-1].copy()
    tile = np.arange(len(seeds)) // 16
    assert (tile[perm] != tile).sum() >= 30                       # all but the middle of the batch change tile
    grad_p, (losses_p, z_p) = hais.grad_and_loss(dev(seeds[perm]), flat, un, fixed, tgt)
    torch.cuda.synchronize()
    where = torch.from_numpy(perm).cuda()
    assert torch.equal(losses_p, losses[where]) and torch.equal(z_p, z[where])
    assert bool(torch.isfinite(grad_p).all())
    compare_grad("UHA floor, reversed", un, grad_p, g_ref)


def test_gradient_of_two_shards_with_n_total(hip_lib):
    """omega = 1 / n_total: the gradients of seeds 1 .. 80 and 81 .. 145, both with n_total = 145, add up to the gradient of
    the whole batch (compared with the float64 one); every shard's losses and end points are the whole call's bits."""
    name, n, K, L = "gmm", 145, 4, 2
    _, _, g_ref = reference(name, K, L, n, with_grad=True)
    flat, un, fixed, _ = built(name, K, L)
    tgt = target_of(name)
    g_all, (l_all, z_all) = hais.grad_and_loss(dev(np.arange(1, n + 1)), flat, un, fixed, tgt)
    g_a, (l_a, z_a) = hais.grad_and_loss(dev(np.arange(1, 81)), flat, un, fixed, tgt, n_total=n)
    g_b, (l_b, z_b) = hais.grad_and_loss(dev(np.arange(81, n + 1)), flat, un, fixed, tgt, n_total=n)
    torch.cuda.synchronize()
    assert torch.equal(l_a, l_all[:80]) and torch.equal(l_b, l_all[80:])
    assert torch.equal(z_a, z_all[:80]) and torch.equal(z_b, z_all[80:])
    compare_grad("gmm shards 80 + 65 of 145", un, g_a.double() + g_b.double(), g_ref)
    assert float((g_a - g_all).abs().max()) > 0                    # a shard alone is not the whole


@pytest.mark.parametrize("name,n,K,L", [("gmm", 37, 8, 3), ("many_gmm", 145, 4, 1), ("funnel", 21, 3, 3)])
def test_doubling_n_total_halves_the_gradient_bit_for_bit(hip_lib, name, n, K, L):
    """Every adjoint of the sweep is homogeneous of degree one in omega and a factor of two is exact in binary floating
    point, in the reduction and through the interpolation too."""
    flat, un, fixed, _ = built(name, K, L)
    seeds = dev(np.arange(1, n + 1))
    g1, (l1, z1) = hais.grad_and_loss(seeds, flat, un, fixed, target_of(name))
    g2, (l2, z2) = hais.grad_and_loss(seeds, flat, un, fixed, target_of(name), n_total=2 * n)
    torch.cuda.synchronize()
    assert float(g1.abs().max()) > 0
    assert torch.equal(g2, 0.5 * g1)
    assert torch.equal(l2, l1) and torch.equal(z2, z1)


def test_only_the_trainable_leaf_carries_a_gradient(hip_lib):
    flat, un, fixed, _ = built("gmm", 8, 1, trainable=("eps",))
    grad, _ = hais.grad_and_loss(dev(np.arange(1, 38)), flat, un, fixed, target_of("gmm"))
    off = un.offset("eps")
    assert (0, "eps") in un.layout and off == 0
    assert float(grad[off]) != 0.0
    rest = torch.cat([grad[:off], grad[off + 1:]])
    assert rest.numel() == flat.numel() - 1 and bool((rest == 0).all())
    # and it is the value the all-trainable tree gets for eps
    flat2, un2, fixed2, _ = built("gmm", 8, 1)
    grad2, _ = hais.grad_and_loss(dev(np.arange(1, 38)), flat2, un2, fixed2, target_of("gmm"))
    assert float(grad2[un2.offset("eps")]) == float(grad[off])


# ------------------------------------------------------------------------------------------ other properties
def _matched_q(name):
    """A q close to (one mode of) the target, so that every loss stays below 16 in magnitude."""
    if name == "gmm":
        return (2.9, 0.1), (0.9, 0.3)
    if name == "funnel":
        return (1.0,) + (0.1,) * 9, (0.5,) + (0.7,) * 9
    from oracle.targets import many_gmm_means
    mu = np.asarray(many_gmm_means(40, 2, 40.0), np.float64)
    return tuple(mu[0] + 0.1), (0.8, 0.7)


@pytest.mark.parametrize("name", ["gmm", "funnel", "many_gmm"])
def test_zero_step_size_is_the_mean_field_bound(hip_lib, name):
    """eps = 0: the chain does not move and its weight terms vanish, so losses and z are the mean-field bound's within 1e-6
    absolute.  The two kernels are compiled separately and may contract a product and a sum differently, one unit in the
    last place; below 16 a float32 is spaced 9.5e-7 or closer, so the bound admits that and nothing more.  Hence a q
    matched to the target: every loss of the case lies inside (-16, 16), which is asserted."""
    dim = TARGETS[name][0]
    seeds = dev(np.arange(1, 38))
    flat, un, fixed = hr.make_params(dim, 8, 2, 0.0, seed=5, device="cuda", vd=_matched_q(name))
    losses, z, _ = hais.bound_forward(seeds, flat, un, fixed, target_of(name))
    _, (l0, z0) = bm.compute_bound(seeds, flat, un, (dim, 0, 1), target_of(name))
    assert float(l0.abs().max()) < 16.0
    print(name, "max |loss difference|", float((losses - l0).abs().max()), "max |z difference|", float((z - z0).abs().max()))
    assert float((losses - l0).abs().max()) <= 1e-6 and float((z - z0).abs().max()) <= 1e-6
    _, (l1, z1) = hais.compute_bound(seeds, flat, un, (dim, 0, 1), target_of(name))      # nbridges = 0 is forwarded
    assert torch.equal(l1, l0) and torch.equal(z1, z0)


@pytest.mark.parametrize("name", ["gmm", "funnel"])
def test_zero_step_size_keeps_the_bits_of_the_mean_field_draw(hip_lib, name):
    """hais_traj_kernel draws z_0 through cmcd_tile.h (tile_split, tile_normal), mfvi_kernel through the inline copy it keeps
    (the note above it in cmcd_mfvi.hip): the two must stay one draw.  With eps = 0 the leap-frog adds eps r / s^2 = 0 to z at
    every step, so the end point of the chain is z_0 = mean + std normal(A) as the mean-field call forms it for the same seeds
    and q: the same bits, on 33 particles (two full tiles and a one-lane tile), K = 2, L = 1, under a q with every leaf
    non-trivial.  The build in which both kernels had private copies satisfied this bit for bit as well
    (profiles/r14_tile_plain_ab.txt, section 3), so nothing is allowed here."""
    dim, _, sigma, mean_scale = TARGETS[name]
    seeds = dev(np.arange(1, 34))
    flat, un, fixed = hr.make_params(dim, 2, 1, 0.0, seed=12, device="cuda", mean_scale=mean_scale, sigma=sigma)
    assert float(flat[un.offset("eps")]) == 0.0 and fixed == (dim, 2, 1)
    _, (_, z) = hais.compute_bound(seeds, flat, un, fixed, target_of(name))
    _, (_, z0) = bm.compute_bound(seeds, flat, un, (dim, 0, 1), target_of(name))       # cmcd_mfvi_bound_grad
    torch.cuda.synchronize()
    assert z.shape == (33, dim) and bool(torch.isfinite(z0).all()) and float(z0.std(dim=0).min()) > 0
    print(name, "entries whose bits differ:", int((z.view(torch.int32) != z0.view(torch.int32)).sum()),
          "max |z difference|", float((z - z0).abs().max()))
    assert torch.equal(z.view(torch.int32), z0.view(torch.int32))


def test_same_bits_forward_gradient_repeat_capture_and_batch_composition(hip_lib):
    name, K, L = "gmm", 8, 3
    flat, un, fixed, _ = built(name, K, L)
    tgt = target_of(name)
    seeds = dev(np.arange(1, 38))
    l_f, z_f, st_f = hais.bound_forward(seeds, flat, un, fixed, tgt)
    g1, (l1, z1) = hais.grad_and_loss(seeds, flat, un, fixed, tgt)
    g2, (l2, z2) = hais.grad_and_loss(seeds, flat, un, fixed, tgt)
    assert torch.equal(l_f, l1) and torch.equal(z_f, z1)          # forward-only call (grad = NULL) == gradient call
    assert torch.equal(g1, g2) and torch.equal(l1, l2)            # repeated calls: the same bits
    # a 74-seed batch: its first 37 particles are the 37-seed call's
    l74, z74, _ = hais.bound_forward(dev(np.arange(1, 75)), flat, un, fixed, tgt)
    assert torch.equal(l74[:37], l_f) and torch.equal(z74[:37], z_f)
    # captured on one stream and replayed
    static = seeds.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        hais.grad_and_loss(static, flat, un, fixed, tgt)          # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        g_c, (l_c, z_c) = hais.grad_and_loss(static, flat, un, fixed, tgt)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(g_c, g1) and torch.equal(l_c, l1) and torch.equal(z_c, z1)
    # 145 particles: three workgroups in the sweep, ten slots in the reduction
    flat4, un4, fixed4, _ = built(name, 4, 2)
    many = dev(np.arange(1, 146))
    g3, (l3, z3) = hais.grad_and_loss(many, flat4, un4, fixed4, tgt)
    g4, (l4, z4) = hais.grad_and_loss(many, flat4, un4, fixed4, tgt)
    torch.cuda.synchronize()
    assert float(g3.abs().max()) > 0
    assert torch.equal(g3, g4) and torch.equal(l3, l4) and torch.equal(z3, z4)


def test_error_paths(hip_lib):
    flat, un, fixed, _ = built("gmm", 8, 1)
    seeds = dev(np.arange(1, 17))
    for fn in (hais.compute_bound, hais.grad_and_loss):
        with pytest.raises(RuntimeError, match="runs on a ROCm device only"):
            fn(seeds, flat.cpu(), un, fixed, target_of("gmm"))
        with pytest.raises(ValueError, match="target dim 10 != params_fixed dim 2"):
            fn(seeds, flat, un, fixed, target_of("funnel"))
        with pytest.raises(ValueError, match="lfsteps"):
            fn(seeds, flat, un, (2, 8, 0), target_of("gmm"))
    from cmcd_amd.lgcp import load_model_lgcp
    from helpers import lgcp_counts_fixture
    lgcp = load_model_lgcp("lgcp", None, flat_bin_counts=lgcp_counts_fixture())[0]
    flat_l, un_l, fixed_l = hais.initialize(lgcp.dim, nbridges=2, eps=0.01, device="cuda")
    with pytest.raises(NotImplementedError, match="lgcp"):
        hais.compute_bound(seeds, flat_l, un_l, fixed_l, lgcp)
    with pytest.raises(NotImplementedError):                      # boundingmachine keeps refusing the chain: it lives in hais
        bm.compute_bound(seeds, flat, un, fixed, target_of("gmm"))


def test_training_lowers_the_bound(hip_lib):
    """opt.run on gmm, K = 8, N = 64, from the reference's start (q = N(0, I), uniform grid) with a small step size: the mean
    loss on 4096 fresh seeds drops by more than 3 standard errors of the difference."""
    import types
    trainable = ("eta", "eps", "vd", "mgridref_y")
    flat, un, fixed = hais.initialize(2, nbridges=8, lfsteps=1, eps=0.01, eta=0.5, trainable=trainable, device="cuda")
    tgt = target_of("gmm")
    fresh = dev(np.arange(2_000_001, 2_000_001 + 4096))
    _, (before, _) = hais.compute_bound(fresh, flat, un, fixed, tgt)
    info = types.SimpleNamespace(N=64)
    _, trained, _ = opt.run(info, 0.005, 300, flat, un, fixed, tgt, hais.grad_and_loss, trainable, 7)
    _, (after, _) = hais.compute_bound(fresh, trained, un, fixed, tgt)
    b, a = before.double().cpu().numpy(), after.double().cpu().numpy()
    assert np.isfinite(b).all() and np.isfinite(a).all()
    se = math.sqrt(b.var(ddof=1) / len(b) + a.var(ddof=1) / len(a))
    print("mean loss before %.4f after %.4f, standard error of the difference %.4f" % (b.mean(), a.mean(), se),
          {k: v.tolist() for k, v in un(trained)[0].items() if not isinstance(v, dict)})
    assert b.mean() - a.mean() > 3 * se
    assert not torch.equal(trained, flat)


@pytest.mark.parametrize("model", ["gmm", "funnel"])
def test_driver_runs_the_default_boundmode(hip_lib, capsys, model):
    from cmcd_amd import main as cli
    cfg = cli.get_config()
    assert cfg.boundmode == "UHA"                                  # the reference's default: no --config.boundmode needed
    argv = ["--config.model", model, "--config.boundmode", "UHA", "--config.N", "16", "--config.nbridges", "4", "--config.lfsteps", "2",
            "--config.mfvi_iters", "20", "--config.iters", "20", "--config.n_samples", "32", "--config.n_input_dist_seeds", "3",
            "--config.init_eps", "0.01", "--config.lr", "0.001"]
    elbo, ln_z = cli.main(cli.parse_flags(argv, cfg))
    out = capsys.readouterr().out
    assert math.isfinite(elbo) and math.isfinite(ln_z)
    assert "Params being trained : ('eta', 'eps', 'vd', 'mgridref_y')" in out
    import re
    for pat in (r"Done training, got ELBO (\S+)\.\n", r"Done training, got ln Z (\S+)\.\n", r"Importance weights behind ln Z: ESS (\S+) "):
        m = re.search(pat, out)
        assert m and math.isfinite(float(m.group(1))), (pat, out)
    assert "Reverse chain" not in out                              # gated to the overdamped MCD modes
    if model == "funnel":
        m = re.search(r"W2 to the target (\S+) ", out)
        assert m and math.isfinite(float(m.group(1))), out
