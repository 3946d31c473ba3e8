"""Mean-field VI (cmcd_amd.boundingmachine, C ABI cmcd_mfvi_bound_grad) on the GPU vs the float64 restatement.

The cases of tests/mfvi_cases.py (its header says which line of cmcd_mfvi.hip / lgcp_mfvi each shape reaches, and
tests/test_oracle_mfvi.py asserts it on the CPU) are held to max(1e-4, 4 x the restatement's own float32 gap) on the worst
particle and on each gradient leaf: a single evaluation has no chain to amplify round-off, so the suite's 1e-3 / 2e-3 would
let through an error a hundred times what float32 explains."""
import types

import numpy as np
import pytest
import torch

from cmcd_amd import boundingmachine as bm
from cmcd_amd import mcdboundingmachine as mcdbm
from cmcd_amd import opt, synthetic
from cmcd_amd.lgcp import load_model_lgcp
from cmcd_amd.model_handler import load_model
from oracle import cmcd_oracle as orc

import mfvi_cases as mc
from helpers import check_stats, compare_losses, lgcp_counts_fixture, oracle_target

pytestmark = pytest.mark.gpu


def _setup(model, n, seed=3):
    rng = np.random.default_rng(seed)
    if model == "lgcp":
        target, dim = load_model_lgcp("lgcp", None, flat_bin_counts=lgcp_counts_fixture())
        mean = np.full(dim, np.log(126.0) - 0.955) + 0.05 * rng.standard_normal(dim)
        logdiag = np.full(dim, np.log(0.5)) + 0.05 * rng.standard_normal(dim)
        otarget = oracle_target({"model": "lgcp"}, lgcp_counts_fixture())
    else:
        target, dim, _ = load_model(model, types.SimpleNamespace())
        sig = 15.0 if model == "many_gmm" else 1.0
        mean = 0.3 * rng.standard_normal(dim)
        logdiag = np.log(sig) + 0.1 * rng.standard_normal(dim)
        otarget = oracle_target({"model": model})
    vdp = {"mean": torch.tensor(mean, dtype=torch.float32), "logdiag": torch.tensor(logdiag, dtype=torch.float32)}
    flat, unflatten, fixed = bm.initialize(dim=dim, nbridges=0, vdparams=vdp, trainable=("vd",), device="cuda")
    vd64 = {k: v.double().numpy() for k, v in vdp.items()}
    return target, otarget, dim, flat, unflatten, fixed, vd64


@pytest.mark.parametrize("model,n", [("gmm", 300), ("funnel", 301), ("many_gmm", 2000), ("many_gmm", 7), ("lgcp", 29)])
def test_mfvi_bound_and_gradient_match_the_oracle(hip_lib, model, n):
    target, otarget, dim, flat, unflatten, fixed, vd64 = _setup(model, n)
    seeds = synthetic.parity_seeds(n)
    grad, (losses, z) = bm.grad_and_loss(torch.from_numpy(seeds).cuda(), flat, unflatten, fixed, target)
    mean, (losses2, z2) = bm.compute_bound(torch.from_numpy(seeds).cuda(), flat, unflatten, fixed, target)
    torch.cuda.synchronize()
    assert torch.equal(losses, losses2) and torch.equal(z, z2)
    l_ref, z_ref = orc.mfvi_losses(seeds, vd64, dim, otarget)
    compare_losses(losses.cpu().numpy(), l_ref, z.cpu().numpy(), z_ref, tag=f"mfvi {model}", K=0)
    assert np.isfinite(l_ref).all(), "a case of this list is finite: the gradient check below is never skipped"
    assert abs(float(mean) - l_ref.mean()) <= 1e-3 * max(1.0, abs(l_ref.mean()))
    g_ref = orc.mfvi_grad(seeds, vd64, dim, otarget)
    g = grad.double().cpu().numpy()
    for leaf in ("mean", "logdiag"):
        off = unflatten.offset("vd", leaf)
        a, r = g[off:off + dim], g_ref[leaf]
        assert np.abs(a - r).max() <= 2e-3 * max(np.abs(r).max(), 1e-3), (leaf, np.abs(a - r).max(), np.abs(r).max())
    other = np.ones(g.shape[0], bool)
    for leaf in ("mean", "logdiag"):
        off = unflatten.offset("vd", leaf)
        other[off:off + dim] = False
    assert not g[other].any()


# ------------------------------------------------------------------------------------------ the cases of tests/mfvi_cases.py
def _dev(seeds):
    return torch.from_numpy(np.ascontiguousarray(seeds, np.int32)).cuda()


def _leaves(unflatten, dim, g):
    """flat gradient (any array type) -> ({leaf: its dim entries}, mask of every other entry)."""
    other = np.ones(len(g), bool)
    out = {}
    for leaf in ("mean", "logdiag"):
        off = unflatten.offset("vd", leaf)
        out[leaf] = g[off:off + dim]
        other[off:off + dim] = False
    return out, other


@pytest.mark.parametrize("cid", mc.IDS)
def test_mfvi_cases_match_the_oracle(hip_lib, cid):
    """Losses, z and the +inf set, both gradient leaves, the statistics with and without the gradient, and compute_bound, on
    every case of tests/mfvi_cases.py.  Worst particle and each leaf: max(1e-4, 4 x float32 gap of the restatement).
    A floored particle (many_gmm below -1e4 nats) has loss +inf, adds 0 to d / d mean and -1 / n to d / d logdiag, so the
    gradient stays finite beside a +inf mean; floor-all's is exactly (0, -1)."""
    case = mc.case_by_id(cid)
    target, otarget, dim, flat, unflatten, fixed, vd64 = mc.build(case, "cuda")[:7]
    seeds = mc.seeds_of(case)
    n = len(seeds)
    l_ref, z_ref, g_ref = mc.reference(case)
    bar_l, bar_g = mc.bars(case)
    grad, losses, z, stats = bm._call(_dev(seeds), flat, unflatten, fixed, target, True)
    _, losses_f, z_f, stats_f = bm._call(_dev(seeds), flat, unflatten, fixed, target, False)
    grad2, (losses2, z2) = bm.grad_and_loss(_dev(seeds), flat, unflatten, fixed, target)
    mean, (losses3, z3) = bm.compute_bound(_dev(seeds), flat, unflatten, fixed, target)
    torch.cuda.synchronize()
    # the forward-only call returns the gradient call's bits, and the public wrappers those of _call
    for l_, z_ in ((losses_f, z_f), (losses2, z2), (losses3, z3)):
        assert torch.equal(losses, l_) and torch.equal(z, z_)
    assert torch.equal(grad, grad2)
    assert losses.shape == (n,) and z.shape == (n, dim)
    l, zz = losses.cpu().numpy(), z.cpu().numpy()
    f = np.isfinite(l_ref)
    if f.any():
        rep = compare_losses(l, l_ref, zz, z_ref, tag=f"mfvi {cid}", K=0, rel_max=bar_l)
        print(f"{cid}: worst particle {rep['rel_max']:.2e} (bar {bar_l:.1e}) z_max {rep['z_max']:.2e}")
    else:       # compare_losses takes its scales from the finite particles: none here
        assert np.array_equal(l, l_ref) and (l == np.inf).all()
        assert np.abs(zz - z_ref).max() <= 1e-3 * max(1.0, float(np.quantile(np.abs(z_ref), 0.99)))
    for st, want_grad in ((stats, True), (stats_f, False)):
        check_stats(st, losses, f"mean-field {cid} grad={want_grad}")
    assert torch.equal(stats, stats_f)
    if f.all():
        assert abs(float(mean) - l_ref.mean()) <= bar_l * max(1.0, abs(l_ref.mean()))
    else:
        assert float(mean) == np.inf
    g = grad.double().cpu().numpy()
    if f.any():
        assert np.isfinite(g).all()
    got, other = _leaves(unflatten, dim, g)
    for leaf in ("mean", "logdiag"):
        err = mc.leaf_error(got[leaf], g_ref[leaf])
        print(f"{cid}: vd/{leaf} {err:.2e} (bar {bar_g[leaf]:.1e})")
        assert err <= bar_g[leaf], (leaf, err, bar_g[leaf], float(np.abs(g_ref[leaf]).max()))
    assert not g[other].any()
    if case[4].get("all_floored"):
        assert np.array_equal(got["mean"], np.zeros(dim)) and np.array_equal(got["logdiag"], -np.ones(dim))
        assert [float(v) for v in stats.cpu()] == [0.0, np.inf, np.inf, -np.inf, 0.0]


@pytest.mark.parametrize("cid,cut", [("gmm-145", 100), ("funnel-133", 100), ("lgcp-65", 33)])
def test_shards_add_up(hip_lib, cid, cut):
    """Multi-GPU contract: two shards called with n_total = the whole batch sum to the single call (the tile kernel applies
    omega = 1 / n_total per lane, lgcp as the scale of the reduction); n_total = 2 n halves the gradient bit for bit; losses, z
    and statistics do not depend on n_total."""
    case = mc.case_by_id(cid)
    target, _, dim, flat, unflatten, fixed, _ = mc.build(case, "cuda")[:7]
    seeds = _dev(mc.seeds_of(case))
    n = seeds.numel()
    args = (flat, unflatten, fixed, target)
    g_all, l_all, z_all, st_all = bm._call(seeds, *args, True)
    g_a, (l_a, z_a) = bm.grad_and_loss(seeds[:cut], *args, n_total=n)
    g_b, (l_b, z_b) = bm.grad_and_loss(seeds[cut:], *args, n_total=n)
    assert float(g_all.abs().max()) > 0
    torch.testing.assert_close(g_a + g_b, g_all, rtol=2e-4, atol=2e-6 * float(g_all.abs().max()))
    assert torch.equal(torch.cat([l_a, l_b]), l_all) and torch.equal(torch.cat([z_a, z_b]), z_all)
    g_half, l_h, z_h, st_h = bm._call(seeds, *args, True, n_total=2 * n)
    assert torch.equal(g_half * 2, g_all)
    assert torch.equal(l_h, l_all) and torch.equal(z_h, z_all) and torch.equal(st_h, st_all)
    g_one, _, _, _ = bm._call(seeds, *args, True, n_total=n)
    assert torch.equal(g_one, g_all)


@pytest.mark.parametrize("cid", ["gmm-145", "floor-half", "lgcp-33"])
def test_repeated_calls_are_bitwise_identical(hip_lib, cid):
    """The per-tile sums (row_sum16, one gradient row per tile) and lgcp's per-particle rows are reduced in a fixed order:
    twenty calls, with an unrelated launch in between, return the same bits."""
    case = mc.case_by_id(cid)
    target, _, dim, flat, unflatten, fixed, _ = mc.build(case, "cuda")[:7]
    seeds = _dev(mc.seeds_of(case))
    first = None
    noise = torch.randn(1 << 20, device="cuda")
    for rep in range(20):
        if rep % 3 == 1:
            noise = noise * 1.0001   # an unrelated launch in between
        out = tuple(t.clone() for t in bm._call(seeds, flat, unflatten, fixed, target, True))
        if first is None:
            first = out
            assert torch.isfinite(out[0]).all()
        else:
            for name, a, b in zip(("grad", "losses", "z", "stats"), out, first):
                assert torch.equal(a, b), (rep, name)


def test_batch_order_does_not_matter(hip_lib):
    """floor-half on its seeds reversed: every particle lands in another lane of another tile, beside other floored and
    unfloored particles, and returns the same loss and z bits."""
    case = mc.case_by_id("floor-half")
    target, _, dim, flat, unflatten, fixed, _, seeds = mc.build(case, "cuda")
    _, (l, z) = bm.grad_and_loss(_dev(seeds), flat, unflatten, fixed, target)
    _, (l_r, z_r) = bm.grad_and_loss(_dev(seeds[::-1]), flat, unflatten, fixed, target)
    assert torch.isinf(l).any() and torch.isfinite(l).any()
    assert torch.equal(l_r.flip(0), l) and torch.equal(z_r.flip(0), z)


def test_untrained_q_gets_a_zero_gradient(hip_lib):
    """trainable = (): "vd" sits in params_notrain, whose gradient _zero_notrain clears (stop_gradient of the reference's
    boundingmachine.py:75); the losses are those of the trainable build."""
    case = mc.case_by_id("gmm-145")
    target, _, dim, flat, unflatten, fixed, _ = mc.build(case, "cuda")
    seeds = _dev(mc.seeds_of(case))
    vdp = {k: torch.from_numpy(v.copy()) for k, v in mc.q_of(case).items()}
    flat0, unflatten0, fixed0 = bm.initialize(dim=dim, nbridges=0, vdparams=vdp, trainable=(), device="cuda")
    g, (l, z) = bm.grad_and_loss(seeds, flat, unflatten, fixed, target)
    g0, (l0, z0) = bm.grad_and_loss(seeds, flat0, unflatten0, fixed0, target)
    assert g.abs().max() > 0 and g0.shape == flat0.shape and not g0.any()
    assert torch.equal(l0, l) and torch.equal(z0, z)


def test_mfvi_draws_the_z0_of_the_mcd_machine(hip_lib):
    """Same key usage (split(PRNGKey(seed))[0] -> sample_rep) in both machines: bit-identical z."""
    b = synthetic.build("many_gmm_n2000_k256_dds", device="cuda", nbridges=1, init_eps=1e-12)
    train, _ = b["unflatten"](b["params_flat"])
    target = b["target"]
    flat, unflatten, fixed = bm.initialize(dim=2, nbridges=0, vdparams={k: v.cpu() for k, v in train["vd"].items()} if "vd" in train
                                           else None, trainable=("vd",), init_sigma=60.0, device="cuda")
    seeds = torch.from_numpy(synthetic.parity_seeds(100)).cuda()
    _, (_, z_mf) = bm.compute_bound(seeds, flat, unflatten, fixed, target)
    l, z, _ = mcdbm.bound_forward(seeds, b["params_flat"], b["unflatten"], b["params_fixed"], target)
    # one step of size ~1e-12 leaves z_1 = z_0 + sqrt(2e-12) * noise: equal to ~1e-5
    assert float((z - z_mf).abs().max()) < 2e-5


def test_mfvi_pretraining_raises_the_elbo(hip_lib):
    """main.py:82-109: opt.run on bm.compute_bound with trainable = ("vd",)."""
    target, dim, _ = load_model("gmm", types.SimpleNamespace())
    flat, unflatten, fixed = bm.initialize(dim=dim, nbridges=0, trainable=("vd",), init_sigma=1.0, device="cuda")
    fresh = torch.from_numpy(synthetic.throughput_seeds(4000, stream=9)).cuda()
    v0 = float(bm.compute_bound(fresh, flat, unflatten, fixed, target)[0])
    losses, flat2, _ = opt.run(types.SimpleNamespace(N=500), 1e-2, 400, flat, unflatten, fixed, target,
                               bm.grad_and_loss, ("vd",), 0)
    v1 = float(bm.compute_bound(fresh, flat2, unflatten, fixed, target)[0])
    print("mean-field -ELBO", v0, "->", v1)
    assert np.isfinite(v1) and v1 < v0 - 0.3


def test_mfvi_unsupported(hip_lib):
    target, dim, _ = load_model("gmm", types.SimpleNamespace())
    flat, unflatten, fixed = bm.initialize(dim=dim, nbridges=4, trainable=("vd",), device="cuda")
    with pytest.raises(NotImplementedError):
        bm.compute_bound(torch.arange(1, 9, dtype=torch.int32).cuda(), flat, unflatten, fixed, target)
    flat, unflatten, fixed = bm.initialize(dim=dim, nbridges=0, trainable=("vd",), device="cpu")
    with pytest.raises(RuntimeError):
        bm.compute_bound(torch.arange(1, 9, dtype=torch.int32), flat, unflatten, fixed, target)
