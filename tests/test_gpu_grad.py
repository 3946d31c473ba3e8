"""Gradients of the HIP path — VarGrad (compute_log_var_grad) and the reparameterised MCD_CAIS_sn gradient
(compute_bound_grad) — vs torch-autograd on the float64 restatement.

The cases, their ids and the float64 references (once per (case, parameter set)) come from tests/grad_blocks.py; every comparison
holds the per-leaf 2e-3 bar and the cosine, and on top of them every block of that file's cut to its own bar."""
import numpy as np
import pytest
import torch

from cmcd_amd import mcdboundingmachine as mcdbm
from cmcd_amd import synthetic
from oracle import cmcd_oracle_torch as ot

import grad_blocks as gb

pytestmark = pytest.mark.gpu


def oracle_grad_flat(b, seeds):
    """The oracle's gradient re-assembled in params_flat order."""
    cfg = b["cfg"]
    dim, K, mode, spec = b["params_fixed"]
    p = synthetic.oracle_params(b["unflatten"], b["params_flat"])
    val, losses, z, g = ot.bound_and_grad(seeds, p, dim, K, mode, spec.arch, cfg["model"], cfg["eps_schedule"],
                                          cfg["grad_clipping"])
    flat = torch.zeros(b["params_flat"].numel(), dtype=torch.float64)
    train, notrain = b["unflatten"](flat)
    allp = {**train, **notrain}
    t = lambda a: torch.as_tensor(np.asarray(a))
    allp["vd"]["mean"].copy_(t(g["vd"]["mean"])); allp["vd"]["logdiag"].copy_(t(g["vd"]["logdiag"]))
    allp["eps"].copy_(t(g["eps"])); allp["mgridref_y"].copy_(t(g["mgridref_y"]))
    if "gamma" in g:   # MCD_CAIS_UHA_sn's friction (zero gradient in every other mode)
        allp["gamma"].copy_(t(g["gamma"]))
    sn, gs = allp["sn"], g["sn"]
    if "nn" in sn:
        (w1, b1), (w2, b2), (w3, b3) = sn["nn"]
        for dst, k in ((w1, "W1"), (b1, "b1"), (w2, "W2"), (b2, "b2"), (w3, "W3"), (b3, "b3")):
            dst.copy_(t(gs[k]))
        sn["emb"].copy_(t(gs["emb"])); sn["factor_sn"].copy_(t(gs["factor_sn"]))
    else:
        m = lambda n: sn["drift_net/~/" + n]
        sn["drift_net"]["timestep_phase"].copy_(t(gs["timestep_phase"]))
        for mod, (wk, bk) in (("linear", ("t_w1", "t_b1")), ("linear_1", ("t_w2", "t_b2")), ("linear_2", ("s_w1", "s_b1")),
                              ("linear_3", ("s_w2", "s_b2")), ("linear_zero", ("s_w3", "s_b3"))):
            m(mod)["w"].copy_(t(gs[wk])); m(mod)["b"].copy_(t(gs[bk]))
    return val, losses, flat


CASES = gb.rows("var")       # (config, particles, overrides): tests/grad_blocks.py, VAR_CASES


@pytest.mark.parametrize("item", [0, 1])
@pytest.mark.parametrize("name,n,over", CASES)
def test_vargrad_matches_autograd(hip_lib, param_set, monkeypatch, name, n, over, item):
    """item = 1: the work-item path (trajectory stored, (tile, evaluation) pairs in parallel); 0: whole chains."""
    monkeypatch.setenv("CMCD_GRAD_ITEM", str(item))
    b = synthetic.build(name, device="cuda", **over)
    seeds = synthetic.parity_seeds(n)
    grad, (losses, z) = mcdbm.compute_log_var_grad(torch.from_numpy(seeds).cuda(), b["params_flat"], b["unflatten"],
                                                   b["params_fixed"], b["target"], eps_schedule=b["eps_schedule"],
                                                   grad_clipping=b["grad_clipping"])
    torch.cuda.synchronize()
    cid = gb.cid_of("var", name, n, over)
    val, l_ref, g_ref = gb.reference_torch(cid, param_set)
    assert np.isfinite(l_ref).all(), "pick a case without +inf particles for the gradient check"
    _compare(name, over, b["unflatten"], grad.double().cpu(), g_ref, blocks=(cid, param_set))


def _compare(name, over, un, g, g_ref, tol=2e-3, blocks=None):
    """`tol`: the bar of every leaf, or {leaf name ("vd/mean", "sn/nn/0/0", ...): bar} for the leaves that have one of their
    own (tests/trained_cases.py) — every other leaf keeps 2e-3.
    `blocks`: (case id, parameter set) of tests/grad_blocks.py — on top of the leaf bars and the cosine, every block of that
    file's cut is held to its own bar (from the stored float32 gap of the restatement, never from `g`)."""
    block_failures = gb.report_blocks(*blocks, un, g, g_ref) if blocks is not None else []
    own = tol if isinstance(tol, dict) else {}
    tol = 2e-3 if isinstance(tol, dict) else tol
    worst = {}
    for path, (off, shape) in un.layout.items():
        numel = max(1, int(np.prod(shape)))
        a, r = g[off:off + numel], g_ref[off:off + numel]
        scale = max(float(r.abs().max()), 1e-12)
        worst["/".join(map(str, path))] = (float((a - r).abs().max()) / scale, scale)
        if float(r.abs().max()) == 0.0:
            assert float(a.abs().max()) == 0.0, f"{path}: expected exactly zero gradient"
    bad = {k: v for k, v in worst.items() if v[0] > own.get(k.split("/", 1)[1], tol) and v[1] > 1e-9}
    print(name, over, {k: "%.1e" % v[0] for k, v in worst.items()})
    assert not bad, f"gradient mismatch (max abs err / max |ref|, max |ref|): {bad}"
    cos = float((g * g_ref).sum() / (g.norm() * g_ref.norm()))
    assert cos > 1 - 1e-5
    assert not block_failures, block_failures


# the reparameterised gradient: no stop_gradient, back-propagation through all K steps
BPTT_CASES = gb.rows("sn")     # tests/grad_blocks.py, BPTT_CASES


@pytest.mark.parametrize("variant,item", [(1, 0), (2, 0), (1, 1), (2, 1), (3, 1)])
@pytest.mark.parametrize("name,n,over", BPTT_CASES)
def test_reparameterised_gradient_matches_autograd(hip_lib, param_set, monkeypatch, name, n, over, variant, item):
    """compute_bound_grad == jax.grad(compute_bound, 1): values from autograd through the float64 restatement
    with no detach (oracle/cmcd_oracle_torch.py).  Both forward kernel variants store the trajectory; item = 0 is
    the sequential reverse sweep, item = 1 the Jacobian + scan + work-item path for small batches."""
    monkeypatch.setattr(mcdbm, "KERNEL_VARIANT", variant)
    monkeypatch.setenv("CMCD_GRAD_ITEM", str(item))
    b = synthetic.build(name, device="cuda", **over)
    assert b["params_fixed"][2] == "MCD_CAIS_sn"
    seeds = synthetic.parity_seeds(n)
    try:
        grad, (losses, z) = mcdbm.compute_bound_grad(torch.from_numpy(seeds).cuda(), b["params_flat"], b["unflatten"],
                                                     b["params_fixed"], b["target"], eps_schedule=b["eps_schedule"],
                                                     grad_clipping=b["grad_clipping"])
    except NotImplementedError as e:
        if variant >= 2 and "cooperative" in str(e):
            pytest.skip("no cooperative instance for this net")
        raise
    torch.cuda.synchronize()
    cid = gb.cid_of("sn", name, n, over)
    val, l_ref, g_ref = gb.reference_torch(cid, param_set)
    assert np.isfinite(l_ref).all(), "pick a case without +inf particles for the gradient check"
    np.testing.assert_allclose(losses.cpu().numpy(), l_ref, rtol=2e-3, atol=2e-3)
    _compare(name, over, b["unflatten"], grad.double().cpu(), g_ref, blocks=(cid, param_set))


@pytest.mark.parametrize("item", [0, 1])
@pytest.mark.parametrize("mode", ["MCD_CAIS_sn", "MCD_CAIS_var_sn"])
@pytest.mark.parametrize("n,K", [(1, 1), (17, 2), (3, 1), (33, 3)])
def test_gradient_edge_shapes(hip_lib, monkeypatch, mode, n, K, item):
    """Single particle, single bridge, ragged last tile — both gradients, both kernel paths, both parameter sets; the flat
    gradient against its largest entry, and every block of tests/grad_blocks.py's cut against its own bar."""
    monkeypatch.setenv("CMCD_GRAD_ITEM", str(item))
    cid = gb.cid_of("edge", "gmm_n300_k8", n, dict(boundmode=mode, nbridges=K))
    for param_set in gb.PARAM_SETS:
        monkeypatch.setattr(synthetic, "DENSE_DEFAULT", param_set == "dense")
        b = synthetic.build("gmm_n300_k8", device="cuda", boundmode=mode, nbridges=K)
        seeds = synthetic.parity_seeds(n)
        fn = mcdbm.compute_bound_grad if mode == "MCD_CAIS_sn" else mcdbm.compute_log_var_grad
        grad, (losses, z) = fn(torch.from_numpy(seeds).cuda(), b["params_flat"], b["unflatten"], b["params_fixed"],
                               b["target"], eps_schedule=b["eps_schedule"], grad_clipping=b["grad_clipping"])
        torch.cuda.synchronize()
        val, l_ref, g_ref = gb.reference_torch(cid, param_set)
        np.testing.assert_allclose(losses.cpu().numpy(), l_ref, rtol=2e-3, atol=2e-3)
        g = grad.double().cpu()
        if n == 1 and mode == "MCD_CAIS_var_sn":
            assert float(g.abs().max()) == 0.0 and float(g_ref.abs().max()) < 1e-12   # variance of one particle
            continue
        scale = float(g_ref.abs().max())
        assert float((g - g_ref).abs().max()) <= 3e-3 * scale, (float((g - g_ref).abs().max()), scale)
        gb.assert_blocks(cid, param_set, b["unflatten"], g, g_ref)


@pytest.mark.parametrize("item", [0, 1])
def test_reparameterised_gradient_shards_add_up(hip_lib, monkeypatch, item):
    """Two particle shards with omega = 1 / N_total sum to the single-call gradient (the multi-GPU contract)."""
    monkeypatch.setenv("CMCD_GRAD_ITEM", str(item))
    b = synthetic.build("many_gmm_n2000_k256_dds", device="cuda", nbridges=12, init_sigma=15.0)
    seeds = torch.from_numpy(synthetic.parity_seeds(200)).cuda()
    args = (b["params_flat"], b["unflatten"], b["params_fixed"], b["target"])
    kw = dict(eps_schedule=b["eps_schedule"], grad_clipping=b["grad_clipping"])
    g_all, _ = mcdbm.compute_bound_grad(seeds, *args, **kw)
    g_a, _ = mcdbm.compute_bound_grad(seeds[:112], *args, n_total=200, **kw)
    g_b, _ = mcdbm.compute_bound_grad(seeds[112:], *args, n_total=200, **kw)
    g_sum = (g_a + g_b).double().cpu()
    g_all = g_all.double().cpu()
    assert float((g_sum - g_all).abs().max()) <= 1e-4 * float(g_all.abs().max())


def test_training_with_the_reparameterised_gradient_raises_the_elbo(hip_lib):
    """opt.run on MCD_CAIS_sn (the reference's default training mode): mean loss on fresh seeds drops."""
    import types
    from functools import partial
    from cmcd_amd import opt
    b = synthetic.build("many_gmm_n2000_k256_dds", device="cuda", nbridges=16, init_sigma=15.0, init_eps=0.3)
    dim, K, mode, spec = b["params_fixed"]
    flat, unflatten, fixed = mcdbm.initialize(
        dim=dim, nbridges=K, vdparams={"mean": torch.zeros(dim), "logdiag": torch.full((dim,), float(np.log(15.0)))},
        eps=0.3, trainable=("eps", "vd", "mgridref_y"), mode=mode, emb_dim=20, nn_arch="dds", device="cuda")
    kw = dict(eps_schedule=b["eps_schedule"], grad_clipping=b["grad_clipping"])
    fresh = torch.from_numpy(synthetic.throughput_seeds(4000, stream=5)).cuda()
    v0 = float(mcdbm.compute_bound(fresh, flat, unflatten, fixed, b["target"], **kw)[0])
    losses, flat2, _ = opt.run(types.SimpleNamespace(N=500), 5e-3, 300, flat, unflatten, fixed, b["target"],
                               partial(mcdbm.compute_bound_grad, **kw), ("eps", "vd", "mgridref_y"), 0)
    v1 = float(mcdbm.compute_bound(fresh, flat2, unflatten, fixed, b["target"], **kw)[0])
    print("mean loss (-ELBO)", v0, "->", v1)
    assert np.isfinite(v1) and v1 < v0 - 0.5


def test_unsupported_configurations_fail_loudly(hip_lib):
    seeds = torch.arange(1, 33, dtype=torch.int32).cuda()
    b = synthetic.build("funnel_n300_k64", device="cuda", boundmode="MCD_CAIS_var_sn", nbridges=4, emb_dim=160)
    with pytest.raises(NotImplementedError):                                          # width 170 > 144: no instance
        mcdbm.compute_log_var_grad(seeds, b["params_flat"], b["unflatten"], b["params_fixed"], b["target"])
    b = synthetic.build("gmm_n300_k8", device="cuda")                                 # MCD_CAIS_sn
    with pytest.raises(NotImplementedError, match="Mode not implemented."):
        mcdbm.compute_log_var_grad(seeds, b["params_flat"], b["unflatten"], b["params_fixed"], b["target"])
    b = synthetic.build("gmm_n300_k8", device="cuda", boundmode="MCD_CAIS_var_sn")    # wrong mode for the full gradient
    with pytest.raises(NotImplementedError, match="Mode not implemented."):
        mcdbm.compute_bound_grad(seeds, b["params_flat"], b["unflatten"], b["params_fixed"], b["target"])
    b = synthetic.build("funnel_n300_k64", device="cuda", nbridges=4, emb_dim=100)                        # funnel beyond 4 tiles
    with pytest.raises(NotImplementedError):
        mcdbm.compute_bound_grad(seeds, b["params_flat"], b["unflatten"], b["params_fixed"], b["target"])


def test_training_with_vargrad_reduces_the_loss(hip_lib):
    """opt.run (Adam + clip + project, reference opt.py:14-35,67-164) driven by compute_log_var_grad: the
    log-variance loss on FRESH seeds must drop and stay finite; non-trainable leaves must not move."""
    import types
    from functools import partial
    from cmcd_amd import opt
    b = synthetic.build("many_gmm_var_n16000_k256", device="cuda", emb_dim=20, nbridges=16, init_sigma=15.0)
    dim, K, mode, spec = b["params_fixed"]
    flat, unflatten, fixed = mcdbm.initialize(
        dim=dim, nbridges=K, vdparams={"mean": torch.zeros(dim), "logdiag": torch.full((dim,), float(np.log(15.0)))},
        eps=0.65, trainable=("eta", "gamma", "mgridref_y"), mode=mode, emb_dim=20, nn_arch="geffner", device="cuda")
    kw = dict(eps_schedule=b["eps_schedule"], grad_clipping=b["grad_clipping"])
    fresh = torch.from_numpy(synthetic.throughput_seeds(4000, stream=5)).cuda()
    v0 = float(mcdbm.compute_bound_var(fresh, flat, unflatten, fixed, b["target"], **kw)[0])
    losses, flat2, _ = opt.run(types.SimpleNamespace(N=1000), 5e-3, 400, flat, unflatten, fixed, b["target"],
                               partial(mcdbm.compute_log_var_grad, **kw), ("eta", "gamma", "mgridref_y"), 0)
    v1 = float(mcdbm.compute_bound_var(fresh, flat2, unflatten, fixed, b["target"], **kw)[0])
    print("log-variance loss", v0, "->", v1)
    assert np.isfinite(v1) and v1 < 0.6 * v0
    _, notrain0 = unflatten(flat)
    _, notrain1 = unflatten(flat2)
    assert torch.equal(notrain0["eps"], notrain1["eps"]) and torch.equal(notrain0["vd"]["mean"], notrain1["vd"]["mean"])
    train1, _ = unflatten(flat2)
    assert float(train1["sn"]["factor_sn"]) != 0.0 and float(train1["mgridref_y"].min()) >= 0.001


def test_fused_optimiser_step_equals_the_eager_one(hip_lib):
    """cmcd_adam_step (clip -> Adam -> apply -> project -> EMA in one launch) == the eager torch arithmetic of
    opt._ClipAdam + opt.project (reference opt.py:14-35,100-116), step by step."""
    from cmcd_amd import opt
    flat, unflatten, _ = mcdbm.initialize(dim=2, nbridges=8, eps=0.4, eta=0.9, gamma=0.002,
                                          trainable=("eps", "eta", "gamma", "mgridref_y"), mode="MCD_CAIS_sn",
                                          nn_arch="geffner", emb_dim=4, device="cuda")
    trainable = ("eps", "eta", "gamma", "mgridref_y")
    g = torch.Generator().manual_seed(0)
    pa, pb = flat.clone(), flat.clone()
    ema_a, ema_b = flat.clone(), flat.clone()
    fused, eager = opt.create_optimizer(0.05), opt._ClipAdam(0.05)
    sa, sb = fused.init(pa), eager.init(pb)
    for it in range(5):
        grad = (torch.randn(flat.numel(), generator=g) * 8.0).cuda()      # some entries beyond the +-5 clip
        fused.step(pa, grad, sa, unflatten, trainable, ema=ema_a)
        upd, sb = eager.update(grad, sb, pb)
        pb.add_(upd)
        opt.project(pb, unflatten, trainable)
        ema_b.mul_(1 - 0.001).add_(pb, alpha=0.001)
        assert float((pa - pb).abs().max()) <= 1e-6 * max(1.0, float(pb.abs().max())), it
        assert float((ema_a - ema_b).abs().max()) <= 1e-6 * max(1.0, float(ema_b.abs().max()))
    train, _ = unflatten(pa)
    assert 1e-7 <= float(train["eps"]) <= 0.5 and 0 <= float(train["eta"]) <= 0.99 and float(train["gamma"]) >= 0.001
    assert float(train["mgridref_y"].min()) >= 0.001


def test_fused_optimiser_step_with_non_finite_input(hip_lib):
    """optax.clip passes NaN through and clips +-inf (the eager torch.clamp does the same); a NaN mean loss skips the
    update and raises the sticky device flag — /root/reference/src/opt.py:122-124 returns before the update."""
    from cmcd_amd import opt
    flat, unflatten, _ = mcdbm.initialize(dim=2, nbridges=4, eps=0.4, trainable=("eps", "mgridref_y"), mode="MCD_CAIS_sn",
                                          nn_arch="geffner", emb_dim=4, device="cuda")
    trainable = ("eps", "mgridref_y")
    n = flat.numel()
    grad = torch.randn(n, generator=torch.Generator().manual_seed(1)).cuda()
    grad[3], grad[5], grad[7] = float("nan"), float("inf"), float("-inf")
    pa, pb = flat.clone(), flat.clone()
    fused, eager = opt.create_optimizer(0.05), opt._ClipAdam(0.05)
    sa, sb = fused.init(pa), eager.init(pb)
    fused.step(pa, grad, sa, unflatten, trainable)
    upd, sb = eager.update(grad, sb, pb)
    pb.add_(upd)
    opt.project(pb, unflatten, trainable)
    assert bool(torch.isnan(pa[3])) and bool(torch.isnan(pb[3]))
    ok = torch.ones(n, dtype=torch.bool, device="cuda")
    ok[3] = False
    assert bool(torch.isfinite(pa[ok]).all()) and float((pa[ok] - pb[ok]).abs().max()) <= 1e-6
    assert bool(torch.isnan(sa["mu"][3])) and float(sa["mu"][5]) == pytest.approx(0.5) and float(sa["mu"][7]) == pytest.approx(-0.5)
    # the guard: a finite or +inf mean loss lets the step through, a NaN one does not and the flag stays up
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    g2 = torch.ones(n, device="cuda")
    for losses, want_skip in ((torch.tensor([1.0, 2.0, float("inf")]), False), (torch.tensor([1.0, float("nan"), 2.0]), True),
                              (torch.tensor([1.0, 2.0, 3.0]), True)):    # the last one: sticky
        p = flat.clone()
        st = fused.init(p)
        fused.step(p, g2, st, unflatten, trainable, losses=losses.cuda(), diverged=flag)
        assert torch.equal(p, flat) == want_skip and (int(flag) != 0) == want_skip
        if want_skip:
            assert float(st["mu"].abs().max()) == 0.0
    flag.zero_()
    p = flat.clone()
    fused.step(p, g2, fused.init(p), unflatten, trainable, losses=torch.tensor([float("inf"), float("-inf")]).cuda(), diverged=flag)
    assert torch.equal(p, flat) and int(flag) == 1          # inf - inf: the mean is NaN


def test_vargrad_weights_follow_the_variance_clip(hip_lib):
    """compute_bound_var returns clip(var, +-1e7) (/root/reference/src/mcdboundingmachine.py:231): inside the clip
    d var / d w_n = -(2 / N)(l_n - mean l); outside jnp.clip passes no gradient, so every weight is zero; a batch with an
    infinite loss has var = NaN and NaN weights, as jax.grad gives."""
    import ctypes as C
    from cmcd_amd import _lib
    from oracle import cmcd_oracle as orc

    def weights(losses):
        l = torch.tensor(losses, dtype=torch.float32, device="cuda")
        stats = torch.tensor(orc.stats5(np.asarray(losses, np.float64)), dtype=torch.float64, device="cuda")
        om = torch.empty_like(l)
        _lib.check(hip_lib.cmcd_vargrad_weights(l.data_ptr(), stats.data_ptr(), l.numel(), l.numel(), om.data_ptr(), None))
        torch.cuda.synchronize()
        return om.cpu().numpy()
    small = np.array([1.0, 2.0, 4.0, 9.0])
    np.testing.assert_allclose(weights(small), -(2.0 / 4) * (small - small.mean()), rtol=1e-6)
    big = np.array([0.0, 1.0e4, -1.0e4, 3.0])                 # var = 5e7 > 1e7
    assert np.var(big) > 1e7 and not weights(big).any()
    edge = np.array([0.0, 6.0e3, -6.0e3, 0.0])                # var = 1.8e7 > 1e7 as well; 4e3 -> 8e6 is inside
    assert not weights(edge).any()
    inside = np.array([0.0, 4.0e3, -4.0e3, 0.0])
    np.testing.assert_allclose(weights(inside), -(2.0 / 4) * (inside - inside.mean()), rtol=1e-6)
    assert np.isnan(weights(np.array([1.0, np.inf, 2.0, 3.0]))).all()


def test_opt_run_stops_at_a_nan_loss_with_the_last_finite_parameters(hip_lib):
    """opt.run polls the divergence flag: a grad_and_loss that turns NaN at iteration 7 leaves the parameters of
    iteration 6 (what /root/reference/src/opt.py:122-124 returns), however rarely the host looks."""
    import types
    from cmcd_amd import opt
    flat, unflatten, fixed = mcdbm.initialize(dim=2, nbridges=4, eps=0.4, trainable=("eps",), mode="MCD_CAIS_sn",
                                              nn_arch="geffner", emb_dim=4, device="cuda")
    calls = {"n": 0, "snap": None}

    def grad_and_loss(seeds, params_flat, *_):
        calls["n"] += 1
        loss = torch.ones(seeds.numel(), device="cuda")
        if calls["n"] == 8:
            calls["snap"] = params_flat.clone()
        if calls["n"] >= 8:
            loss[0] = float("nan")
        return torch.full_like(params_flat, 0.3), (loss, None)
    _, out, _ = opt.run(types.SimpleNamespace(N=16), 1e-2, 5000, flat, unflatten, fixed, None, grad_and_loss, ("eps",), 0)
    assert calls["n"] < 5000 and calls["snap"] is not None and torch.equal(out, calls["snap"])
    assert not torch.equal(out, flat)


@pytest.mark.parametrize("mode", ["MCD_CAIS_sn", "MCD_CAIS_var_sn", "MCD_CAIS_UHA_sn"])
def test_graph_replayed_training_equals_eager_training(hip_lib, mode):
    """opt.run with the iteration captured in a HIP graph (static seed buffer, device-side Adam step count) ends
    where the eager loop ends, from the same seeds."""
    import types
    from cmcd_amd import opt
    b = synthetic.build("gmm_n300_k8", device="cuda", boundmode=mode)
    dim, K, _, spec = b["params_fixed"]
    flat, unflatten, fixed = mcdbm.initialize(dim=dim, nbridges=K, eps=0.01, trainable=("eps", "vd", "mgridref_y"),
                                              mode=mode, emb_dim=20, nn_arch="geffner", device="cuda")
    gl, _ = mcdbm.make_grad_and_loss(mode, eps_schedule=b["eps_schedule"], grad_clipping=b["grad_clipping"])
    out = {}
    for use_graph in (False, True):
        losses, p, ema = opt.run(types.SimpleNamespace(N=300), 1e-3, 60, flat, unflatten, fixed, b["target"], gl,
                                 ("eps", "vd", "mgridref_y"), 7, use_ema=True, use_graph=use_graph)
        out[use_graph] = (np.array(losses), p.double().cpu(), ema.double().cpu())
    assert float((out[True][1] - out[False][1]).abs().max()) <= 2e-5 * max(1.0, float(out[False][1].abs().max()))
    assert float((out[True][2] - out[False][2]).abs().max()) <= 2e-5 * max(1.0, float(out[False][2].abs().max()))
    np.testing.assert_allclose(out[True][0], out[False][0], rtol=1e-4, atol=1e-4)
    assert float((out[True][1] - flat.double().cpu()).abs().max()) > 1e-3      # and it did train


@pytest.mark.parametrize("form", [0, 3], ids=["kept_activations", "split_k_recompute"])
@pytest.mark.parametrize("n,K,clip", [(5, 3, False), (37, 2, True), (20, 2, True)])
def test_lgcp_reparameterised_gradient_matches_autograd(hip_lib, param_set, monkeypatch, n, K, clip, form):
    """d = 1600 (config 5): launch-sequence reverse sweep + deferred A^T B parameter contractions vs autograd
    through the float64 restatement.  n = 37 spans two passes of 32 and 5 particles, n = 20 is the named batch's pass (16 + 4
    rows per workgroup).  form 0 (r04): the forward's consumers keep every evaluation's activations and the sweep runs on the
    no-split-K GEMM where a pass has <= 20 particles (the 32-particle pass: kept activations, split-K products); form 3 pins
    the split-K kernels, whose sweep recomputes each evaluation on a side stream (rounds 1 - 3)."""
    from helpers import lgcp_counts_fixture
    if form == 3 and n == 20:
        pytest.skip("the recompute form is covered by the two other shapes (suite time)")
    monkeypatch.setattr(mcdbm, "KERNEL_VARIANT", form)
    counts = lgcp_counts_fixture()
    b = synthetic.build("lgcp_n20_k128", device="cuda", lgcp_counts=counts, nbridges=K, N=n, grad_clipping=clip,
                        init_eps=2e-3)
    assert b["params_fixed"][2] == "MCD_CAIS_sn"
    seeds = synthetic.parity_seeds(n)
    grad, (losses, z) = mcdbm.compute_bound_grad(torch.from_numpy(seeds).cuda(), b["params_flat"], b["unflatten"],
                                                 b["params_fixed"], b["target"], eps_schedule=b["eps_schedule"],
                                                 grad_clipping=b["grad_clipping"])
    torch.cuda.synchronize()
    dim, _, mode, spec = b["params_fixed"]
    p = synthetic.oracle_params(b["unflatten"], b["params_flat"])
    val, l_ref, z_ref, g = ot.bound_and_grad(seeds, p, dim, K, mode, spec.arch, ot.make_logp_lgcp(counts),
                                             b["cfg"]["eps_schedule"], clip)
    np.testing.assert_allclose(losses.cpu().numpy(), l_ref, rtol=2e-4, atol=0.5)
    un = b["unflatten"]
    gh = grad.double().cpu().numpy()

    def leaf(*path):
        off, shape = un.layout[(0,) + path] if (0,) + path in un.layout else un.layout[(1,) + path]
        return gh[off:off + max(1, int(np.prod(shape)))].reshape(shape)
    (w1, b1), (w2, b2), (w3, b3) = [(("sn", "nn", i, 0), ("sn", "nn", i, 1)) for i in range(3)]
    checks = {"vd.mean": (leaf("vd", "mean"), g["vd"]["mean"]), "vd.logdiag": (leaf("vd", "logdiag"), g["vd"]["logdiag"]),
              "eps": (leaf("eps"), g["eps"]), "mgridref_y": (leaf("mgridref_y"), g["mgridref_y"]),
              "W1": (leaf(*w1), g["sn"]["W1"]), "b1": (leaf(*b1), g["sn"]["b1"]), "W2": (leaf(*w2), g["sn"]["W2"]),
              "b2": (leaf(*b2), g["sn"]["b2"]), "W3": (leaf(*w3), g["sn"]["W3"]), "b3": (leaf(*b3), g["sn"]["b3"]),
              "emb": (leaf("sn", "emb"), g["sn"]["emb"]), "factor_sn": (leaf("sn", "factor_sn"), g["sn"]["factor_sn"])}
    worst = {}
    for name, (a, r) in checks.items():
        r = np.asarray(r, np.float64).reshape(a.shape)
        scale = max(np.abs(r).max(), 1e-12)
        worst[name] = (float(np.abs(a - r).max() / scale), float(scale))
    print({k: "%.1e (|ref| %.1e)" % v for k, v in worst.items()})
    bad = {k: v for k, v in worst.items() if v[0] > 5e-3 and v[1] > 1e-9}
    assert not bad, bad


@pytest.mark.parametrize("n,K,clip", [(6, 3, False), (37, 2, True)])
def test_lgcp_vargrad_matches_autograd(hip_lib, param_set, n, K, clip):
    """d = 1600 with MCD_CAIS_var_sn: the reverse launch sequence with z detached (no lambda recursion, no Hessian
    product), per-particle weights from the statistics — against autograd of var(losses) through the float64
    restatement with the reference's stop_gradient placement.  n = 37 spans two passes; clip = 1e2 on both scores."""
    from helpers import lgcp_counts_fixture
    counts = lgcp_counts_fixture()
    b = synthetic.build("lgcp_n20_k128", device="cuda", lgcp_counts=counts, nbridges=K, N=n, grad_clipping=clip,
                        init_eps=2e-3, boundmode="MCD_CAIS_var_sn")
    assert b["params_fixed"][2] == "MCD_CAIS_var_sn"
    seeds = synthetic.parity_seeds(n)
    grad, (losses, z) = mcdbm.compute_log_var_grad(torch.from_numpy(seeds).cuda(), b["params_flat"], b["unflatten"],
                                                   b["params_fixed"], b["target"], eps_schedule=b["eps_schedule"],
                                                   grad_clipping=b["grad_clipping"])
    torch.cuda.synchronize()
    dim, _, mode, spec = b["params_fixed"]
    p = synthetic.oracle_params(b["unflatten"], b["params_flat"])
    val, l_ref, z_ref, g = ot.bound_and_grad(seeds, p, dim, K, mode, spec.arch, ot.make_logp_lgcp(counts),
                                             b["cfg"]["eps_schedule"], clip)
    np.testing.assert_allclose(losses.cpu().numpy(), l_ref, rtol=2e-4, atol=0.5)
    un = b["unflatten"]
    gh = grad.double().cpu().numpy()

    def leaf(*path):
        off, shape = un.layout[(0,) + path] if (0,) + path in un.layout else un.layout[(1,) + path]
        return gh[off:off + max(1, int(np.prod(shape)))].reshape(shape)
    (w1, b1), (w2, b2), (w3, b3) = [(("sn", "nn", i, 0), ("sn", "nn", i, 1)) for i in range(3)]
    checks = {"vd.mean": (leaf("vd", "mean"), g["vd"]["mean"]), "vd.logdiag": (leaf("vd", "logdiag"), g["vd"]["logdiag"]),
              "eps": (leaf("eps"), g["eps"]), "mgridref_y": (leaf("mgridref_y"), g["mgridref_y"]),
              "W1": (leaf(*w1), g["sn"]["W1"]), "b1": (leaf(*b1), g["sn"]["b1"]), "W2": (leaf(*w2), g["sn"]["W2"]),
              "b2": (leaf(*b2), g["sn"]["b2"]), "W3": (leaf(*w3), g["sn"]["W3"]), "b3": (leaf(*b3), g["sn"]["b3"]),
              "emb": (leaf("sn", "emb"), g["sn"]["emb"]), "factor_sn": (leaf("sn", "factor_sn"), g["sn"]["factor_sn"])}
    worst = {}
    for name, (a, r) in checks.items():
        r = np.asarray(r, np.float64).reshape(a.shape)
        scale = max(np.abs(r).max(), 1e-12)
        worst[name] = (float(np.abs(a - r).max() / scale), float(scale))
    print({k: "%.1e (|ref| %.1e)" % v for k, v in worst.items()})
    # float32 losses of size ~300 enter the weights 2 (l_p - mean) / n: the relative error of a weight is ~1e-4
    bad = {k: v for k, v in worst.items() if v[0] > 5e-3 and v[1] > 1e-9}
    assert not bad, bad


ULA_CASES = [c[1:] for c in gb.ULA_CASES]     # tests/grad_blocks.py: ids "ulasn-*" with the network, "ula-*" without


@pytest.mark.parametrize("variant,item", [(1, 0), (2, 1), (1, 1)])
@pytest.mark.parametrize("name,n,over", ULA_CASES)
def test_ula_sn_gradient_matches_autograd(hip_lib, param_set, monkeypatch, name, n, over, variant, item):
    """MCD_ULA_sn (the "MCD" baseline, /root/reference/src/mcd_over_orig.py): network only in the backward kernel
    with index i, constant eps, no clipping — same reverse recursion, through both gradient paths."""
    monkeypatch.setattr(mcdbm, "KERNEL_VARIANT", variant)
    monkeypatch.setenv("CMCD_GRAD_ITEM", str(item))
    b = synthetic.build(name, device="cuda", boundmode="MCD_ULA_sn", **over)
    seeds = synthetic.parity_seeds(n)
    grad, (losses, z) = mcdbm.compute_bound_grad(torch.from_numpy(seeds).cuda(), b["params_flat"], b["unflatten"],
                                                 b["params_fixed"], b["target"], eps_schedule=b["eps_schedule"],
                                                 grad_clipping=b["grad_clipping"])
    torch.cuda.synchronize()
    cid = gb.cid_of("ulasn", name, n, over)
    val, l_ref, g_ref = gb.reference_torch(cid, param_set)
    assert np.isfinite(l_ref).all()
    np.testing.assert_allclose(losses.cpu().numpy(), l_ref, rtol=2e-3, atol=2e-3)
    _compare(name, over, b["unflatten"], grad.double().cpu(), g_ref, blocks=(cid, param_set))


@pytest.mark.parametrize("name,n,over", ULA_CASES)
def test_ula_gradient_matches_autograd(hip_lib, param_set, name, n, over):
    """MCD_ULA (no network): gradient w.r.t. eps, the schedule grid and q through the network-free reverse sweep."""
    b = synthetic.build(name, device="cuda", boundmode="MCD_ULA", **over)
    seeds = synthetic.parity_seeds(n)
    grad, (losses, z) = mcdbm.compute_bound_grad(torch.from_numpy(seeds).cuda(), b["params_flat"], b["unflatten"],
                                                 b["params_fixed"], b["target"])
    torch.cuda.synchronize()
    dim, K, mode, _ = b["params_fixed"]
    flat = b["params_flat"].detach().cpu()
    train, notrain = b["unflatten"](flat)
    allp = {**train, **notrain}
    f = lambda t: np.asarray(t.numpy(), np.float64)
    p = {"vd": {k: f(v) for k, v in allp["vd"].items()}, "eps": f(allp["eps"]), "mgridref_y": f(allp["mgridref_y"]),
         "gridref_x": f(allp["gridref_x"]), "target_x": f(allp["target_x"])}
    val, l_ref, _, g = ot.bound_and_grad(seeds, p, dim, K, mode, "dds", b["cfg"]["model"], None, False)
    np.testing.assert_allclose(losses.cpu().numpy(), l_ref, rtol=2e-3, atol=2e-3)
    un, gh = b["unflatten"], grad.double().cpu().numpy()
    for path, ref in ((("vd", "mean"), g["vd"]["mean"]), (("vd", "logdiag"), g["vd"]["logdiag"]), (("eps",), g["eps"]),
                      (("mgridref_y",), g["mgridref_y"])):
        off = un.offset(*path)
        ref = np.asarray(ref, np.float64).reshape(-1)
        got = gh[off:off + ref.size]
        assert np.abs(got - ref).max() <= 2e-3 * max(np.abs(ref).max(), 1e-9), (path, got, ref)
    cid = gb.cid_of("ula", name, n, over)
    gb.assert_blocks(cid, param_set, un, gh, gb.reference(cid, param_set)[3])


@pytest.mark.parametrize("mode,n,K", [("MCD_ULA_sn", 6, 3), ("MCD_ULA", 37, 3)])
def test_lgcp_overdamped_baselines_match_autograd(hip_lib, param_set, mode, n, K):
    """d = 1600 with the two overdamped baselines (mcd_over_orig.py): MCD_ULA_sn = network in the backward kernel only,
    time index i; MCD_ULA = no network at all (one GEMM launch per evaluation forward, two per evaluation in the reverse
    sweep).  Losses and every gradient leaf against autograd through the float64 restatement."""
    from helpers import lgcp_counts_fixture
    counts = lgcp_counts_fixture()
    b = synthetic.build("lgcp_n20_k128", device="cuda", lgcp_counts=counts, nbridges=K, N=n, init_eps=2e-3, boundmode=mode)
    seeds = synthetic.parity_seeds(n)
    grad, (losses, z) = mcdbm.compute_bound_grad(torch.from_numpy(seeds).cuda(), b["params_flat"], b["unflatten"],
                                                 b["params_fixed"], b["target"])
    torch.cuda.synchronize()
    dim, _, _, spec = b["params_fixed"]
    un = b["unflatten"]
    if mode == "MCD_ULA":
        train, notrain = un(b["params_flat"].detach().cpu())
        allp = {**train, **notrain}
        f = lambda t: np.asarray(t.numpy(), np.float64)
        p = {"vd": {k: f(v) for k, v in allp["vd"].items()}, "eps": f(allp["eps"]), "mgridref_y": f(allp["mgridref_y"]),
             "gridref_x": f(allp["gridref_x"]), "target_x": f(allp["target_x"])}
        arch = "geffner"
    else:
        p = synthetic.oracle_params(un, b["params_flat"])
        arch = spec.arch
    val, l_ref, z_ref, g = ot.bound_and_grad(seeds, p, dim, K, mode, arch, ot.make_logp_lgcp(counts), None, False)
    np.testing.assert_allclose(losses.cpu().numpy(), l_ref, rtol=2e-4, atol=0.5)
    np.testing.assert_allclose(z.cpu().numpy(), z_ref, rtol=0, atol=5e-4)
    gh = grad.double().cpu().numpy()

    def leaf(*path):
        off, shape = un.layout[(0,) + path] if (0,) + path in un.layout else un.layout[(1,) + path]
        return gh[off:off + max(1, int(np.prod(shape)))].reshape(shape)
    checks = {"vd.mean": (leaf("vd", "mean"), g["vd"]["mean"]), "vd.logdiag": (leaf("vd", "logdiag"), g["vd"]["logdiag"]),
              "eps": (leaf("eps"), g["eps"]), "mgridref_y": (leaf("mgridref_y"), g["mgridref_y"])}
    if mode == "MCD_ULA_sn":
        (w1, b1), (w2, b2), (w3, b3) = [(("sn", "nn", i, 0), ("sn", "nn", i, 1)) for i in range(3)]
        checks.update({"W1": (leaf(*w1), g["sn"]["W1"]), "b1": (leaf(*b1), g["sn"]["b1"]), "W2": (leaf(*w2), g["sn"]["W2"]),
                       "b2": (leaf(*b2), g["sn"]["b2"]), "W3": (leaf(*w3), g["sn"]["W3"]), "b3": (leaf(*b3), g["sn"]["b3"]),
                       "emb": (leaf("sn", "emb"), g["sn"]["emb"]), "factor_sn": (leaf("sn", "factor_sn"), g["sn"]["factor_sn"])})
    worst = {}
    for name, (a, r) in checks.items():
        r = np.asarray(r, np.float64).reshape(a.shape)
        scale = max(np.abs(r).max(), 1e-12)
        worst[name] = (float(np.abs(a - r).max() / scale), float(scale))
    print({k: "%.1e (|ref| %.1e)" % v for k, v in worst.items()})
    bad = {k: v for k, v in worst.items() if v[0] > 5e-3 and v[1] > 1e-9}
    assert not bad, bad


@pytest.mark.parametrize("mode", ["MCD_CAIS_sn", "MCD_CAIS_var_sn"])
def test_sharded_grad_and_loss_without_a_process_group_is_the_plain_call(hip_lib, mode):
    from cmcd_amd import parallel
    b = synthetic.build("gmm_n300_k8", device="cuda", boundmode=mode)
    seeds = torch.from_numpy(synthetic.parity_seeds(100)).cuda()
    args = (seeds, b["params_flat"], b["unflatten"], b["params_fixed"], b["target"])
    gl = parallel.make_sharded_grad_and_loss(mode, eps_schedule=b["eps_schedule"], grad_clipping=b["grad_clipping"])
    plain, _ = mcdbm.make_grad_and_loss(mode, eps_schedule=b["eps_schedule"], grad_clipping=b["grad_clipping"])
    g1, (l1, _) = gl(*args)
    g2, (l2, _) = plain(*args)
    assert torch.equal(l1, l2)
    assert float((g1 - g2).abs().max()) <= 1e-5 * float(g2.abs().max())


@pytest.mark.parametrize("item", [0, 1])
def test_gradient_with_a_17_component_mixture(hip_lib, param_set, monkeypatch, item):
    """The generic component loop of the target's gradient + Hessian (n_mixes != 40)."""
    from functools import partial
    monkeypatch.setenv("CMCD_GRAD_ITEM", str(item))
    b = synthetic.build("many_gmm_n2000_k256_dds", device="cuda", nbridges=6, n_mixes=17, init_sigma=15.0, init_eps=0.3)
    seeds = synthetic.parity_seeds(80)
    grad, (losses, z) = mcdbm.compute_bound_grad(torch.from_numpy(seeds).cuda(), b["params_flat"], b["unflatten"],
                                                 b["params_fixed"], b["target"], eps_schedule=b["eps_schedule"],
                                                 grad_clipping=b["grad_clipping"])
    torch.cuda.synchronize()
    dim, K, mode, spec = b["params_fixed"]
    p = synthetic.oracle_params(b["unflatten"], b["params_flat"])
    val, l_ref, _, g = ot.bound_and_grad(seeds, p, dim, K, mode, spec.arch, partial(ot.logp_many_gmm, n_mixes=17),
                                         b["cfg"]["eps_schedule"], b["cfg"]["grad_clipping"])
    assert np.isfinite(l_ref).all()
    np.testing.assert_allclose(losses.cpu().numpy(), l_ref, rtol=2e-3, atol=2e-3)
    off = b["unflatten"].offset("sn", "drift_net/~/linear_3", "w")
    got = grad[off:off + 4096].double().cpu().numpy().reshape(64, 64)
    ref = np.asarray(g["sn"]["s_w2"])
    assert np.abs(got - ref).max() <= 2e-3 * np.abs(ref).max()
    for leaf in ("mean", "logdiag"):
        off = b["unflatten"].offset("vd", leaf)
        assert np.abs(grad[off:off + 2].double().cpu().numpy() - g["vd"][leaf]).max() <= 2e-3 * np.abs(g["vd"][leaf]).max()
    cid = gb.MIX17_CASE[0]
    assert gb.MIX17_CASE[1:] == ("many_gmm_n2000_k256_dds", 80, dict(nbridges=6, n_mixes=17, init_sigma=15.0, init_eps=0.3))
    gb.assert_blocks(cid, param_set, b["unflatten"], grad, gb.reference(cid, param_set)[3])


# ---------------------------------------------------------------------------------------------- the gated cases
# tests/gated_cases.py: inputs at which the target floor, the score clip and the dds output clamp ACT (asserted on the CPU
# in tests/test_oracle_grad.py).  Same bars as everywhere else in this file.
import gated_cases as gc

_GATED_ORACLE = {}


def gated_oracle(case, param_set):
    """(built case on the device, (value, losses, flat gradient) of the float64 oracle), once per (case, parameter set)."""
    key = (case[0], param_set)
    if key not in _GATED_ORACLE:
        b = gc.build_case(case, device="cuda")
        _GATED_ORACLE[key] = (b, oracle_grad_flat(b, np.asarray(case[3], np.int32)))
    return _GATED_ORACLE[key]


def compare_losses_with_inf(losses, l_ref):
    """The loss check of this file (2e-3) on the finite particles; the +inf particles must be the same set; no NaN."""
    l = np.asarray(losses, np.float64)
    assert not np.isnan(l).any(), "NaN loss"
    assert np.array_equal(np.isinf(l), np.isinf(l_ref)) and not (l == -np.inf).any(), (l, l_ref)
    f = np.isfinite(l_ref)
    np.testing.assert_allclose(l[f], l_ref[f], rtol=2e-3, atol=2e-3)


def gated_call(b, case):
    fn = mcdbm.compute_log_var_grad if case[4] == "MCD_CAIS_var_sn" else mcdbm.compute_bound_grad
    seeds = torch.from_numpy(np.asarray(case[3], np.int32)).cuda()
    grad, (losses, z) = fn(seeds, b["params_flat"], b["unflatten"], b["params_fixed"], b["target"],
                           eps_schedule=b["eps_schedule"], grad_clipping=b["grad_clipping"])
    torch.cuda.synchronize()
    return grad, losses


def assert_paths_agree(out, un):
    """The bars of test_gpu_fullsize.test_work_item_and_whole_chain_gradients_agree_on_a_large_batch."""
    assert torch.equal(out[0][1], out[1][1])
    ga, gb = out[0][0], out[1][0]
    assert float((ga * gb).sum() / (ga.norm() * gb.norm())) > 1 - 1e-8
    for path, (off, shape) in un.layout.items():
        numel = max(1, int(np.prod(shape)))
        a, r = ga[off:off + numel], gb[off:off + numel]
        scale = float(r.abs().max())
        if scale > 1e-9:
            assert float((a - r).abs().max()) <= 2e-4 * scale, (path, float((a - r).abs().max()), scale)


_GATED_PATHS = {"MCD_CAIS_sn": [(1, 0), (2, 0), (1, 1), (2, 1), (3, 1)], "MCD_CAIS_var_sn": [(None, 0), (None, 1)],
                "MCD_ULA_sn": [(1, 0), (2, 1), (1, 1)]}
_GATED_RUNS = [pytest.param(c, v, i, id=f"{c[0]}-variant{v}-item{i}")
               for c in gc.cases_of(*_GATED_PATHS) for v, i in _GATED_PATHS[c[4]]]


@pytest.mark.parametrize("case,variant,item", _GATED_RUNS)
def test_gradient_where_a_gate_acts_matches_autograd(hip_lib, param_set, monkeypatch, case, variant, item):
    """Every leaf against autograd where floored particles, clipped scores or clamped network outputs make a derivative
    exactly zero: both gradient paths, the three forward variants of MCD_CAIS_sn, both parameter sets."""
    if variant is not None:
        monkeypatch.setattr(mcdbm, "KERNEL_VARIANT", variant)
    monkeypatch.setenv("CMCD_GRAD_ITEM", str(item))
    b, (val, l_ref, g_ref) = gated_oracle(case, param_set)
    assert b["params_fixed"][2] == case[4]
    try:
        grad, losses = gated_call(b, case)
    except NotImplementedError as e:
        if variant is not None and variant >= 2 and "cooperative" in str(e):
            pytest.skip("no cooperative instance for this net")
        raise
    compare_losses_with_inf(losses.cpu().numpy(), l_ref)
    if case[0] == "floor-end":
        assert np.isinf(l_ref).any() and bool(torch.isfinite(grad).all())
    _compare(case[0], case[2], b["unflatten"], grad.double().cpu(), g_ref, blocks=("gated-" + case[0], param_set))


@pytest.mark.parametrize("case", gc.cases_of(*_GATED_PATHS), ids=lambda c: c[0])
def test_gradient_paths_agree_where_a_gate_acts(hip_lib, param_set, monkeypatch, case):
    b, _ = gated_oracle(case, param_set)
    out = {}
    for item in (0, 1):
        monkeypatch.setenv("CMCD_GRAD_ITEM", str(item))
        grad, losses = gated_call(b, case)
        assert bool(torch.isfinite(grad).all())
        out[item] = (grad.double().cpu(), losses.cpu())
    assert_paths_agree(out, b["unflatten"])


def test_vargrad_with_an_infinite_loss_is_nan_where_the_finite_batch_has_a_gradient(hip_lib, monkeypatch):
    """many_gmm at sigma_0 = 60, 33 particles, one of them beyond the floor at z_K: var(losses) is NaN and so is every weight
    (test_vargrad_weights_follow_the_variance_clip), so jax.grad returns NaN wherever the gradient is not structurally zero:
    NaN at every entry that is non-zero on the finite sub-batch, exactly zero on every leaf that is exactly zero there.  opt.run
    on such a batch stops as it does on a NaN loss."""
    import types
    from cmcd_amd import opt
    b = synthetic.build("many_gmm_var_n16000_k256", device="cuda", nbridges=4, init_sigma=60.0, emb_dim=20)
    seeds = torch.from_numpy(synthetic.parity_seeds(33)).cuda()
    args = (b["params_flat"], b["unflatten"], b["params_fixed"], b["target"])
    kw = dict(eps_schedule=b["eps_schedule"], grad_clipping=b["grad_clipping"])
    for item in (0, 1):
        monkeypatch.setenv("CMCD_GRAD_ITEM", str(item))
        g_all, (l_all, _) = mcdbm.compute_log_var_grad(seeds, *args, **kw)
        inf = torch.isinf(l_all)
        assert 1 <= int(inf.sum()) < 33 and not bool(torch.isnan(l_all).any())
        g_fin, (l_fin, _) = mcdbm.compute_log_var_grad(seeds[~inf], *args, **kw)
        assert bool(torch.isfinite(l_fin).all()) and bool(torch.isfinite(g_fin).all())
        g_all, g_fin = g_all.cpu(), g_fin.cpu()
        touched = 0
        for path, (off, shape) in b["unflatten"].layout.items():
            numel = max(1, int(np.prod(shape)))
            a, r = g_all[off:off + numel], g_fin[off:off + numel]
            if float(r.abs().max()) == 0.0:
                assert float(a.abs().max()) == 0.0, f"{path}: expected exactly zero gradient"   # NaN fails this too
            else:
                touched += 1
                assert bool(torch.isnan(a[r != 0]).all()), f"{path}: finite entries where jax.grad returns NaN"
        assert touched >= 4
    calls = {"n": 0}

    def grad_and_loss(_, params_flat, *rest):
        calls["n"] += 1
        return mcdbm.compute_log_var_grad(seeds, params_flat, *rest, **kw)
    opt.run(types.SimpleNamespace(N=33), 1e-3, 5000, b["params_flat"], b["unflatten"], b["params_fixed"], b["target"],
            grad_and_loss, ("eps", "vd", "mgridref_y"), 0)
    assert calls["n"] < 5000


REPEAT_CASES = [
    # (synthetic config, particles, overrides, gradient function, CMCD_GRAD_ITEM)
    ("gmm_n300_k8", 300, dict(), "compute_bound_grad", 0),
    ("gmm_n300_k8", 300, dict(), "compute_bound_grad", 1),
    ("gmm_n300_k8", 2000, dict(boundmode="MCD_CAIS_var_sn"), "compute_log_var_grad", 0),
    ("gmm_n300_k8", 300, dict(boundmode="MCD_CAIS_var_sn"), "compute_log_var_grad", 1),
    ("many_gmm_n2000_k256_dds", 500, dict(nbridges=12, init_sigma=15.0), "compute_bound_grad", 1),
    ("many_gmm_n2000_k256_dds", 500, dict(nbridges=12, init_sigma=15.0, nn_arch="geffner", emb_dim=100), "compute_bound_grad", 0),
    ("gmm_n300_k8", 333, dict(boundmode="MCD_ULA_sn"), "compute_bound_grad", 1),
    ("gmm_n300_k8", 333, dict(boundmode="MCD_ULA"), "compute_bound_grad", 0),
    ("gated:floor-mid", 33, None, "compute_bound_grad", 0),        # floored particles (tests/gated_cases.py)
    ("gated:clamp-dds-gmm", 17, None, "compute_bound_grad", 1),    # clamped network outputs
]


@pytest.mark.parametrize("name,n,over,fn,item", REPEAT_CASES)
def test_repeated_gradient_calls_are_bitwise_identical(hip_lib, monkeypatch, name, n, over, fn, item):
    """The sums over particles behind d bias-table / d beta / d eps go through one slot per (tile, evaluation) and a
    fixed-order reduction (cmcd_grad.hip: GradArgs::det, grad_det_reduce_kernel); rounds 1-3 used float atomics on the
    shared tables and the same call returned gradients that differed in the last bits from run to run.  Twenty calls
    with other launches in between (so the waves of the gradient kernel do not arrive in one fixed order)."""
    monkeypatch.setenv("CMCD_GRAD_ITEM", str(item))
    if name.startswith("gated:"):
        case = gc.case_by_id(name[len("gated:"):])
        b = gc.build_case(case, device="cuda")
        seeds = torch.from_numpy(np.asarray(case[3], np.int32)).cuda()
        assert seeds.numel() == n
    else:
        b = synthetic.build(name, device="cuda", **over)
        seeds = torch.from_numpy(synthetic.parity_seeds(n)).cuda()
    call = getattr(mcdbm, fn)
    kw = dict(eps_schedule=b["eps_schedule"], grad_clipping=b["grad_clipping"])
    first = None
    noise = torch.randn(1 << 20, device="cuda")
    for rep in range(20):
        if rep % 3 == 1:
            noise = noise * 1.0001   # an unrelated launch in between
        grad, (losses, _) = call(seeds, b["params_flat"], b["unflatten"], b["params_fixed"], b["target"], **kw)
        g, l = grad.clone(), losses.clone()
        if first is None:
            first = (g, l)
            assert torch.isfinite(g).all()
        else:
            assert torch.equal(g, first[0]), (rep, float((g - first[0]).abs().max()))
            assert torch.equal(l, first[1])


def test_a_training_seed_reproduces_bit_for_bit(hip_lib):
    """Two opt.run trainings with one seed end at the same parameters, bit for bit (gmm K = 8 is chaotic enough that
    last-bit differences in a gradient moved the trained ELBO by 0.05 nats between runs before: tools/probes/
    train_determinism.py, CHANGELOG.md (DESIGN r04 section 6))."""
    import types
    from functools import partial
    from cmcd_amd import opt
    b = synthetic.build("gmm_n300_k8", device="cuda")
    dim, K, mode, spec = b["params_fixed"]
    kw = dict(eps_schedule=b["eps_schedule"], grad_clipping=b["grad_clipping"])
    trainable = ("eps", "vd", "eta", "mgridref_y")
    ends = []
    for _ in range(2):
        flat, unflatten, fixed = mcdbm.initialize(
            dim=dim, nbridges=K, vdparams={"mean": torch.zeros(dim), "logdiag": torch.zeros(dim)}, eps=0.01,
            trainable=trainable, mode=mode, emb_dim=20, nn_arch="geffner", device="cuda", seed=1)
        losses, flat2, _ = opt.run(types.SimpleNamespace(N=300), 1e-3, 300, flat, unflatten, fixed, b["target"],
                                   partial(mcdbm.compute_bound_grad, **kw), trainable, 7)
        ends.append((flat2.clone(), torch.as_tensor(losses).clone()))
    assert torch.isfinite(ends[0][0]).all()
    assert torch.equal(ends[0][0], ends[1][0])
    assert torch.equal(ends[0][1], ends[1][1])
