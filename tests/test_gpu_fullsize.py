"""BASELINE.json's full sizes: size-independent properties of the HIP path (the oracle is too slow
to re-run some of these in seconds, so they rest on determinism, batch-composition invariance,
statistics consistency and the float32 oracle where it is affordable)."""
import math
from functools import partial

import numpy as np
import pytest
import torch

from cmcd_amd import mcdboundingmachine as mcdbm
from cmcd_amd import parallel, synthetic, utils
from oracle import cmcd_oracle as orc

from helpers import check_stats, compare_losses, run_oracle

pytestmark = pytest.mark.gpu


def _fwd(b, seeds):
    s = torch.as_tensor(seeds).cuda()
    out = mcdbm.bound_forward(s, b["params_flat"], b["unflatten"], b["params_fixed"], b["target"],
                              eps_schedule=b["eps_schedule"], grad_clipping=b["grad_clipping"])
    torch.cuda.synchronize()
    return out


def test_north_star_full_batch_against_oracle(hip_lib, param_set):
    """config 3 at its named size (N = 2000, K = 256) vs the float32 reference-faithful oracle (~6 s)."""
    b = synthetic.build("many_gmm_n2000_k256_dds", device="cuda")
    seeds = synthetic.throughput_seeds(2000)
    losses, z, stats = _fwd(b, seeds)
    l_ref, z_ref = run_oracle(b, seeds, dtype=np.float32, reuse=False)
    rep = compare_losses(losses.cpu().numpy(), l_ref, z.cpu().numpy(), z_ref, tag="config 3 full", K=b["params_fixed"][1])
    assert rep["n_inf"] > 0                                     # init_sigma = 60 leaves particles beyond the floor
    lh = losses.double().cpu().numpy()
    assert abs(orc.ln_z(lh) - orc.ln_z(l_ref)) < 0.05           # BASELINE.json's ln Z bar
    check_stats(stats, losses, "config 3 full")                   # all five against float64, n_finite and the maximum exactly
    assert abs(float(mcdbm.ln_z_from_stats(stats, 2000)) - orc.ln_z(lh)) < 1e-9


@pytest.mark.parametrize("name,n", [("many_gmm_n2000_k256_dds", 2000), ("many_gmm_var_n16000_k256", 16000),
                                    ("funnel_n300_k64", 300), ("gmm_n300_k8", 300)])
def test_determinism_and_batch_composition_invariance(hip_lib, monkeypatch, name, n):
    """Same seeds -> bitwise identical losses; a particle's loss does not depend on which batch
    (or which kernel variant's tile) it was launched in."""
    b = synthetic.build(name, device="cuda")
    seeds = synthetic.throughput_seeds(n, stream=5)
    perm = np.random.default_rng(0).permutation(n)
    for v in (1, 3, 4) if n <= 2048 else (1, 3):   # bitwise claims hold per kernel variant and tiling (2 / auto pick the tiling by batch size)
        monkeypatch.setattr(mcdbm, "KERNEL_VARIANT", v)
        l1, z1, s1 = _fwd(b, seeds)
        l2, z2, s2 = _fwd(b, seeds)
        assert torch.equal(l1, l2) and torch.equal(z1, z2) and torch.equal(s1.nan_to_num(1.0), s2.nan_to_num(1.0))
        lp, zp, _ = _fwd(b, seeds[perm])
        assert torch.equal(lp.cpu(), l1.cpu()[perm]) and torch.equal(zp.cpu(), z1.cpu()[perm])
        ls, _, _ = _fwd(b, seeds[37:37 + 101])
        assert torch.equal(ls.cpu(), l1.cpu()[37:37 + 101])
    # both kernel variants compute the same arithmetic per particle up to reduction order
    outs = []
    for v in (1, 2, 3):   # wave per tile, cooperative (8-particle tiles where instantiated), cooperative on 16-particle tiles
        monkeypatch.setattr(mcdbm, "KERNEL_VARIANT", v)
        outs.append(_fwd(b, seeds[:512])[0].double().cpu().numpy())
    f = np.isfinite(outs[0])
    for o in outs[1:]:
        assert np.array_equal(f, np.isfinite(o))
        rel = np.abs(outs[0][f] - o[f]) / np.maximum(1, np.abs(outs[0][f]))
        assert np.quantile(rel, 0.99) < 5e-3


def test_vargrad_config_full_batch_statistics(hip_lib, param_set):
    """config 4 (N = 16000, K = 256, 132-wide net): the returned scalar is var(ddof=0) of the returned
    per-particle losses, statistics agree with torch reductions, and a 64-particle slice agrees with
    the float64 oracle."""
    b = synthetic.build("many_gmm_var_n16000_k256", device="cuda")
    seeds = synthetic.throughput_seeds(16000)
    val, (losses, z) = mcdbm.compute_bound_var(torch.from_numpy(seeds).cuda(), b["params_flat"], b["unflatten"],
                                               b["params_fixed"], b["target"], eps_schedule=b["eps_schedule"],
                                               grad_clipping=b["grad_clipping"])
    torch.cuda.synchronize()
    lh = losses.double()
    assert torch.isfinite(lh).all()
    want = min(1e7, float(lh.var(unbiased=False)))
    assert abs(float(val) - want) <= 1e-6 * want
    l_ref, z_ref = run_oracle(b, seeds[:64], dtype=np.float64)
    compare_losses(losses[:64].cpu().numpy(), l_ref, z[:64].cpu().numpy(), z_ref, tag="config 4 slice", K=b["params_fixed"][1])
    # ... and the WHOLE batch against the reference-faithful float32 C restatement (oracle/cmcd_oracle.c, OpenMP over particles:
    # 16 000 x 256 bridges x two 132-wide evaluations, ~15 s on the GPU box's host cores): every particle's loss and z_K
    from helpers import run_c_oracle
    lc, zc = run_c_oracle(b, seeds)
    rep = compare_losses(losses.cpu().numpy(), lc, z.cpu().numpy(), zc, tag="config 4 full batch vs C oracle", K=b["params_fixed"][1])
    print("config 4 full batch:", rep)


def test_sharded_statistics_equal_single_launch(hip_lib):
    """Running the batch as 8 contiguous shards and merging the 5-number statistics (what 8 ranks do)
    gives the single-launch mean / ln Z."""
    b = synthetic.build("many_gmm_n2000_k256_dds", device="cuda", init_sigma=15.0)
    seeds = synthetic.throughput_seeds(2000, stream=2)
    l_all, _, s_all = _fwd(b, seeds)
    rows = []
    for r in range(8):
        lo, hi = parallel.shard_range(2000, 8, r)
        rows.append(_fwd(b, seeds[lo:hi])[2])
    merged = parallel.merge_stats(torch.stack(rows))                 # device merge kernel
    merged_cpu = parallel.merge_stats(torch.stack(rows).cpu())       # torch-op merge (gloo path)
    np.testing.assert_allclose(merged.cpu().numpy(), merged_cpu.numpy(), rtol=1e-13)
    fa, fb = parallel.finalize(merged, 2000), parallel.finalize(s_all, 2000)
    for k in ("mean", "ln_z", "n_finite"):
        assert abs(float(fa[k]) - float(fb[k])) <= 1e-9 * max(1.0, abs(float(fb[k])))


def test_eval_harness_and_final_metrics(hip_lib):
    """opt.sample + utils.log_final_losses (the numbers the paper reports) on 30 x 500 seeds."""
    b = synthetic.build("gmm_n300_k8", device="cuda", init_sigma=2.0)
    loss_fn = partial(mcdbm.compute_bound, eps_schedule=b["eps_schedule"], grad_clipping=b["grad_clipping"])
    seeds = torch.from_numpy(synthetic.throughput_seeds(30 * 500, stream=11)).cuda()
    elbos, zs = utils.sample(None, 500, 30, b["params_flat"], b["unflatten"], b["params_fixed"], b["target"],
                             loss_fn, seeds)
    assert elbos.shape == (30, 500) and zs.shape == (15000, 2)
    elbo, ln_z = utils.log_final_losses(elbos.cpu())
    e = elbos.double().cpu().numpy()
    assert abs(elbo - (-e.mean(1)).mean()) < 1e-9
    assert abs(ln_z - np.mean([orc.ln_z(r) for r in e])) < 1e-9
    assert abs(ln_z) < 0.2 and elbo < ln_z + 0.05               # normalised target: ln Z ~ 0 >= ELBO


def test_error_paths_on_device(hip_lib):
    b = synthetic.build("gmm_n300_k8", device="cuda")
    dim, K, _, spec = b["params_fixed"]
    seeds = torch.arange(1, 17, dtype=torch.int32).cuda()
    with pytest.raises(NotImplementedError, match="Mode not implemented."):
        mcdbm.compute_bound(seeds, b["params_flat"], b["unflatten"], (dim, K, "MCD_U_a-lp-sn", spec), b["target"])
    with pytest.raises(ValueError):
        mcdbm.compute_bound(seeds[:0], b["params_flat"], b["unflatten"], b["params_fixed"], b["target"])
    from cmcd_amd.model_handler import load_model
    with pytest.raises(ValueError):   # funnel target (d = 10) against a d = 2 parameter set
        mcdbm.compute_bound(seeds, b["params_flat"], b["unflatten"], b["params_fixed"], load_model("funnel")[0])
    int64_seeds = torch.arange(1, 17).cuda()                    # accepted, converted to int32
    a = mcdbm.compute_bound(int64_seeds, b["params_flat"], b["unflatten"], b["params_fixed"], b["target"])[1][0]
    c = mcdbm.compute_bound(seeds, b["params_flat"], b["unflatten"], b["params_fixed"], b["target"])[1][0]
    assert torch.equal(a, c)


@pytest.mark.parametrize("mode", ["MCD_CAIS_sn", "MCD_CAIS_var_sn"])
def test_full_length_gradient_against_autograd(hip_lib, mode):
    """The named chain length (K = 256, dds net, many_gmm, clipping on, cos_sq schedule) through both training
    gradients, 256 particles: float32 kernels vs float64 autograd through the restatement.  Over 256 steps the two
    precisions drift apart particle by particle, so the bar is on the aggregated gradient: cosine > 0.9999 and every
    leaf within 2 % of its scale (measured: 0.8 % reparameterised, 0.02 % VarGrad)."""
    from oracle import cmcd_oracle_torch as ot
    from test_gpu_grad import oracle_grad_flat
    b = synthetic.build("many_gmm_n2000_k256_dds", device="cuda", boundmode=mode, init_sigma=15.0, dense=True)
    assert b["params_fixed"][1] == 256
    seeds = synthetic.parity_seeds(256)
    fn = mcdbm.compute_bound_grad if mode == "MCD_CAIS_sn" else mcdbm.compute_log_var_grad
    grad, (losses, z) = fn(torch.from_numpy(seeds).cuda(), b["params_flat"], b["unflatten"], b["params_fixed"],
                           b["target"], eps_schedule=b["eps_schedule"], grad_clipping=b["grad_clipping"])
    torch.cuda.synchronize()
    val, l_ref, g_ref = oracle_grad_flat(b, seeds)
    assert np.isfinite(l_ref).all()
    g = grad.double().cpu()
    cos = float((g * g_ref).sum() / (g.norm() * g_ref.norm()))
    worst = 0.0
    for path, (off, shape) in b["unflatten"].layout.items():
        numel = max(1, int(np.prod(shape)))
        a, r = g[off:off + numel], g_ref[off:off + numel]
        scale = float(r.abs().max())
        if scale > 1e-9:
            worst = max(worst, float((a - r).abs().max()) / scale)
    print(mode, "cosine", cos, "worst leaf error / scale", worst)
    assert cos > 0.9999 and worst < 2e-2


@pytest.mark.parametrize("mode", ["MCD_CAIS_sn", "MCD_CAIS_var_sn", "MCD_CAIS_UHA_sn"])
def test_work_item_and_whole_chain_gradients_agree_on_a_large_batch(hip_lib, monkeypatch, mode):
    """N = 6000 (ragged last tile), K = 256: the two gradient paths are different kernels and launch sequences of the
    same arithmetic; they must agree to float32 accumulation noise.  (2nd-order mode: the work-item path is the Jacobian
    launch + composite-map scan + chain-chunk sweep of cmcd_uha.hip, 94 quads x 6 chunks here.)"""
    over = dict(init_eps=0.2, init_gamma=2.0) if mode == "MCD_CAIS_UHA_sn" else {}
    b = synthetic.build("many_gmm_n2000_k256_dds", device="cuda", boundmode=mode, init_sigma=15.0, **over)
    seeds = torch.from_numpy(synthetic.throughput_seeds(6000 - 7, stream=3)).cuda()
    fn = mcdbm.compute_log_var_grad if mode == "MCD_CAIS_var_sn" else mcdbm.compute_bound_grad
    out = {}
    for item in ("0", "1"):
        monkeypatch.setenv("CMCD_GRAD_ITEM", item)
        g, (l, z) = fn(seeds, b["params_flat"], b["unflatten"], b["params_fixed"], b["target"],
                       eps_schedule=b["eps_schedule"], grad_clipping=b["grad_clipping"])
        torch.cuda.synchronize()
        out[item] = (g.double().cpu(), l.cpu())
    assert torch.equal(out["0"][1], out["1"][1])
    fin = torch.isfinite(out["0"][1])
    assert bool(fin.all()), "sigma = 15 keeps every particle inside the floor"
    ga, gb = out["0"][0], out["1"][0]
    cos = float((ga * gb).sum() / (ga.norm() * gb.norm()))
    assert cos > 1 - 1e-8, cos
    for path, (off, shape) in b["unflatten"].layout.items():
        numel = max(1, int(np.prod(shape)))
        a, r = ga[off:off + numel], gb[off:off + numel]
        scale = float(r.abs().max())
        if scale > 1e-9:
            assert float((a - r).abs().max()) <= 2e-4 * scale, (path, float((a - r).abs().max()), scale)


@pytest.mark.parametrize("n,k,reps", [(20, 128, 200), (600, 8, 30)])
def test_lgcp_repeat_calls_are_bitwise_identical(hip_lib, n, k, reps):
    """Config 5 at its own size, the same call `reps` times: forward and both gradients must return bit-identical
    results every time.  The d = 1600 launch sequence is the only path with inter-workgroup communication (8 K-slice
    workgroups of a column block count arrivals on a device counter, the last one sums the partial slabs in fixed
    order and runs the fused consumer, cmcd_lgcp.hip): a missing release / acquire would show up as a stale slab,
    i.e. as a run-to-run difference."""
    from helpers import lgcp_counts_fixture
    b = synthetic.build("lgcp_n20_k128", device="cuda", lgcp_counts=lgcp_counts_fixture(), nbridges=k, N=n, dense=True)
    seeds = torch.from_numpy(synthetic.throughput_seeds(n, stream=4)).cuda()
    args = (b["params_flat"], b["unflatten"], b["params_fixed"], b["target"])
    l0, z0, s0 = mcdbm.bound_forward(seeds, *args)
    torch.cuda.synchronize()
    assert torch.isfinite(l0).all()
    for r in range(reps):
        l, z, st = mcdbm.bound_forward(seeds, *args)
        assert torch.equal(l, l0) and torch.equal(z, z0) and torch.equal(st, s0), f"forward repeat {r} differs"
    g0, (lg0, _) = mcdbm.compute_bound_grad(seeds, *args)
    torch.cuda.synchronize()
    assert torch.isfinite(g0).all()
    if n < 224:
        assert torch.equal(lg0, l0)
    else:
        # r04: a forward-only call of >= 224 particles takes the wide-batch GEMM launches (cmcd_lgcp_wide.hip) while a
        # gradient call keeps the trajectory on 32-row passes: the same losses up to the float32 summation order
        torch.testing.assert_close(lg0, l0, rtol=2e-5, atol=2e-3)
    for r in range(max(reps // 4, 10)):
        g, (lg, _) = mcdbm.compute_bound_grad(seeds, *args)
        assert torch.equal(lg, lg0) and torch.equal(g, g0), f"gradient repeat {r} differs"
    # the VarGrad sweep of the same sequence
    bv = synthetic.build("lgcp_n20_k128", device="cuda", lgcp_counts=lgcp_counts_fixture(), nbridges=k, N=n, dense=True,
                         boundmode="MCD_CAIS_var_sn")
    argv = (bv["params_flat"], bv["unflatten"], bv["params_fixed"], bv["target"])
    v0, (lv0, _) = mcdbm.compute_log_var_grad(seeds, *argv)
    for r in range(10):
        v, (lv, _) = mcdbm.compute_log_var_grad(seeds, *argv)
        assert torch.equal(lv, lv0) and torch.equal(v, v0), f"VarGrad repeat {r} differs"
    # batch-composition invariance across GEMM passes: a particle's loss does not depend on its row / pass
    if n > 64:
        perm = torch.from_numpy(np.random.default_rng(1).permutation(n)).cuda()
        lp, _, _ = mcdbm.bound_forward(seeds[perm], *args)
        assert torch.equal(lp, l0[perm])


@pytest.mark.parametrize("name,n", [("many_gmm_n2000_k256_dds", 2000), ("gmm_n300_k8", 300), ("funnel_n300_k64", 300),
                                    ("many_gmm_var_n16000_k256", 600)])
def test_prepared_tables_are_reused_only_while_the_parameters_are_unchanged(hip_lib, monkeypatch, name, n):
    """Evaluation loops on fixed parameters (the reference's opt.sample: 30 loss_fn calls on one params_flat,
    /root/reference/src/opt.py:185-190) skip the per-call prep launch (cmcd_bound_forward_prepared): the results must be
    bit-identical to a full call, and ANY change of the inputs the tables are made of must bring the prep launch back —
    in-place torch updates (version counter), the fused optimiser step (raw-pointer write + manual bump), another batch
    size, another parameter tensor.  gmm / funnel at N = 300 also exercise the fused statistics merge, whose arrival
    counter the prep launch used to zero."""
    from cmcd_amd import opt
    b = synthetic.build(name, device="cuda", nbridges=16) if n == 600 else synthetic.build(name, device="cuda")
    seeds = torch.from_numpy(synthetic.throughput_seeds(n, stream=3)).cuda()
    args = (b["unflatten"], b["params_fixed"], b["target"])
    kw = dict(eps_schedule=b["eps_schedule"], grad_clipping=b["grad_clipping"])
    p = b["params_flat"].clone()
    monkeypatch.setattr(mcdbm, "PREP_CACHE", True)         # what `with mcdbm.fixed_parameters():` does for a loop

    def fresh(params):      # the same call with the cache off
        mcdbm.PREP_CACHE = False
        try:
            return mcdbm.bound_forward(seeds, params, *args, **kw)
        finally:
            mcdbm.PREP_CACHE = True

    def calls():
        return dict(mcdbm.PREP_CALLS)

    l0, z0, s0 = fresh(p)
    c0 = calls()
    outs = [mcdbm.bound_forward(seeds, p, *args, **kw) for _ in range(6)]
    c1 = calls()
    assert c1["full"] - c0["full"] == 1 and c1["prepared"] - c0["prepared"] == 5
    for l, z, st in outs:
        assert torch.equal(l, l0) and torch.equal(z, z0) and torch.equal(st, s0)
    # an in-place update through torch: version counter -> full call, new values
    p.mul_(1.001)
    c1 = calls()
    l1, z1, s1 = mcdbm.bound_forward(seeds, p, *args, **kw)
    assert calls()["full"] - c1["full"] == 1
    lf, zf, sf = fresh(p)
    assert torch.equal(l1, lf) and torch.equal(s1, sf) and not torch.equal(l1, l0)
    # the fused optimiser step writes through raw pointers and bumps the counter by hand
    optimizer = opt.create_optimizer(1e-3)
    state = optimizer.init(p)
    mcdbm.bound_forward(seeds, p, *args, **kw)                      # tables of the current values are in the workspace
    optimizer.step(p, torch.full_like(p, 0.5), state, b["unflatten"], ("eps", "vd", "mgridref_y", "eta", "gamma"))
    c1 = calls()
    l2, _, s2 = mcdbm.bound_forward(seeds, p, *args, **kw)
    assert calls()["full"] - c1["full"] == 1
    lf, _, sf = fresh(p)
    assert torch.equal(l2, lf) and torch.equal(s2, sf)
    # another batch size, then another tensor with the same contents at another address
    c1 = calls()
    mcdbm.bound_forward(seeds[: n // 2], p, *args, **kw)
    mcdbm.bound_forward(seeds, p.clone(), *args, **kw)
    assert calls()["full"] - c1["full"] == 2


@pytest.mark.parametrize("name,n", [("gmm_n300_k8", 300), ("many_gmm_n2000_k256_dds", 2000)])
def test_a_call_outside_the_context_retires_the_prepared_tables(hip_lib, name, n):
    """r04 advisor: `with fixed_parameters(): f(P)`; then OUTSIDE the context f(Q) (or f(P) at another batch size) on the same
    stream — its prep launch overwrites the workspace's tables; then `with fixed_parameters(): f(P)` again.  The third call
    must run its prep launch ('full') and return f(P), not P's chain on Q's tables."""
    b = synthetic.build(name, device="cuda", nbridges=16)
    seeds = torch.from_numpy(synthetic.throughput_seeds(n, stream=5)).cuda()
    args = (b["unflatten"], b["params_fixed"], b["target"])
    kw = dict(eps_schedule=b["eps_schedule"], grad_clipping=b["grad_clipping"])
    P = b["params_flat"].clone()
    Q = (b["params_flat"] * 1.01).contiguous()
    ref_p = [t.clone() for t in mcdbm.bound_forward(seeds, P, *args, **kw)]
    ref_q = [t.clone() for t in mcdbm.bound_forward(seeds, Q, *args, **kw)]
    assert not torch.equal(ref_p[0], ref_q[0])
    for other in ("other parameters", "other batch size", "other eps schedule"):
        with mcdbm.fixed_parameters():
            mcdbm.bound_forward(seeds, P, *args, **kw)
            c = dict(mcdbm.PREP_CALLS)
            got = mcdbm.bound_forward(seeds, P, *args, **kw)
            assert mcdbm.PREP_CALLS["prepared"] - c["prepared"] == 1          # the shortcut is live inside the context
            assert torch.equal(got[0], ref_p[0])
        if other == "other parameters":
            lq = mcdbm.bound_forward(seeds, Q, *args, **kw)[0]
            assert torch.equal(lq, ref_q[0])
        elif other == "other batch size":
            mcdbm.bound_forward(seeds[: n // 2], P, *args, **kw)
        else:
            mcdbm.bound_forward(seeds, P, *args, eps_schedule="linear", grad_clipping=kw["grad_clipping"])
        with mcdbm.fixed_parameters():
            c = dict(mcdbm.PREP_CALLS)
            got = mcdbm.bound_forward(seeds, P, *args, **kw)
            assert mcdbm.PREP_CALLS["full"] - c["full"] == 1, other          # the claim on the buffer was retired
            for g, r in zip(got, ref_p):
                assert torch.equal(g, r), other


@pytest.mark.parametrize("name,n", [("gmm_n300_k8", 300), ("many_gmm_n2000_k256_dds", 2000), ("many_gmm_n2000_k256_dds", 5000)])
def test_the_prepared_entry_point_refuses_tables_of_another_call(hip_lib, name, n):
    """cmcd_bound_forward_prepared's contract, checked on the device (include/cmcd_hip.h): the forming call leaves a stamp of
    its (desc, layout, n, n_params, n_target) in the workspace; a prepared call with another n or descriptor gets NaN statistics
    ("diverged") instead of silent garbage.  Covers the fused merge (38 workgroups), the finalize launch behind the cooperative
    kernel (250) and behind the wave-per-tile kernel (n = 5000)."""
    import ctypes as C
    from cmcd_amd import _lib
    L = _lib.lib()
    b = synthetic.build(name, device="cuda", nbridges=8)
    dim, K, mode, spec = b["params_fixed"]
    un = b["unflatten"]
    seeds = torch.from_numpy(synthetic.throughput_seeds(n, stream=9).astype(np.int32)).cuda()
    consts = b["target"].consts_on(torch.device("cuda"))
    cp, cn = (consts.data_ptr(), consts.numel()) if consts is not None else (None, 0)

    def desc(eps_schedule):
        return _lib.Desc(dim=dim, nbridges=K, mode=_lib.MODE[mode], arch=_lib.ARCH[spec.arch], emb_dim=spec.emb_dim,
                         target=b["target"].target_id, eps_schedule=eps_schedule, grad_clipping=int(bool(b["grad_clipping"])),
                         ngrid=un.shape("mgridref_y")[0] - 1, reserved=0)
    d0 = desc(_lib.EPS_SCHEDULE[b["eps_schedule"]])
    lay = mcdbm._layout(un, spec)
    ws = torch.empty(L.cmcd_workspace_bytes(C.byref(d0), n) + 4096, dtype=torch.uint8, device="cuda")
    p = b["params_flat"]

    def call(fn, d, m):
        loss = torch.empty(m, dtype=torch.float32, device="cuda")
        z = torch.empty(m, dim, dtype=torch.float32, device="cuda")
        st = torch.empty(5, dtype=torch.float64, device="cuda")
        _lib.check(fn(C.byref(d), C.byref(lay), seeds.data_ptr(), m, p.data_ptr(), p.numel(), cp, cn, ws.data_ptr(), ws.numel(),
                      loss.data_ptr(), z.data_ptr(), st.data_ptr(), torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        return loss, st
    l0, s0 = call(L.cmcd_bound_forward, d0, n)
    l1, s1 = call(L.cmcd_bound_forward_prepared, d0, n)              # the contract kept: same bits
    assert torch.equal(l0, l1) and torch.equal(s0, s1) and not torch.isnan(s1).any()
    _, s2 = call(L.cmcd_bound_forward_prepared, d0, n - 8)           # another batch size on these tables
    assert torch.isnan(s2).all()
    other = desc((d0.eps_schedule + 1) % 3)
    _, s3 = call(L.cmcd_bound_forward_prepared, other, n)            # another descriptor
    assert torch.isnan(s3).all()
    _, s4 = call(L.cmcd_bound_forward_prepared, d0, n)               # and the right one still passes afterwards
    assert torch.equal(s4, s0)


def test_the_boundary_only_library_runs_the_path_and_the_bench(hip_lib):
    """cmcd_amd/libcmcd_hip_boundary.so (-DCMCD_NO_DIAG_HOOKS, built by __graft_entry__.build()): no measurement / diagnostic
    export, and the Python boundary and bench.py run on it — same losses, bit for bit, as the in-tree library; bench.py's
    kernel time falls back to the wall time per step."""
    import json
    import os
    import subprocess
    import sys
    from cmcd_amd import build
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = build.build_boundary_only()
    code = (
        "import sys, numpy as np, torch\n"
        f"sys.path.insert(0, {root!r})\n"
        "from cmcd_amd import _lib, synthetic\n"
        "from cmcd_amd import mcdboundingmachine as mcdbm\n"
        "b = synthetic.build('gmm_n300_k8', device='cuda')\n"
        "seeds = torch.from_numpy(synthetic.parity_seeds(300)).cuda()\n"
        "l, z, st = mcdbm.bound_forward(seeds, b['params_flat'], b['unflatten'], b['params_fixed'], b['target'],\n"
        "                               eps_schedule=b['eps_schedule'], grad_clipping=b['grad_clipping'])\n"
        "torch.cuda.synchronize()\n"
        "L = _lib.lib()\n"
        "print('HAS_DIAG', _lib.HAS_DIAG, hasattr(L, 'cmcd_profile_enable'), hasattr(L, 'cmcd_debug_capture_noise'), hasattr(L, 'cmcd_bound_forward'))\n"
        "print('SUM', repr(float(l.double().sum())), repr(float(z.double().sum())))\n")
    env = dict(os.environ, CMCD_LIB_PATH=lib)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "HAS_DIAG False False False True" in out.stdout, out.stdout
    b = synthetic.build("gmm_n300_k8", device="cuda")
    l, z, _ = _fwd(b, synthetic.parity_seeds(300))
    want = f"SUM {float(l.double().sum())!r} {float(z.double().sum())!r}"
    assert want in out.stdout, (want, out.stdout)
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--config", "gmm_n300_k8", "--steps", "5", "--warmup", "2",
                          "--full", "--no-cpu-baseline", "--saturated", "0", "--no-legs"], capture_output=True, text=True,
                         timeout=600, cwd=root, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    r = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][0])
    assert r["value"] > 0 and r["roofline"]["kernel"] == "" and r["roofline"]["kernel_ms"] == pytest.approx(r["ms_per_step"], rel=0.35)


def test_a_captured_forward_keeps_its_prep_launch(hip_lib, monkeypatch):
    """A forward call captured into a HIP graph must carry its prep launch (the prepared-table shortcut is refused while a
    stream is capturing): replays after an in-place parameter update have to see the new parameters."""
    monkeypatch.setattr(mcdbm, "PREP_CACHE", True)
    b = synthetic.build("gmm_n300_k8", device="cuda")
    seeds = torch.from_numpy(synthetic.throughput_seeds(300, stream=5)).cuda()
    args = (b["unflatten"], b["params_fixed"], b["target"])
    kw = dict(eps_schedule=b["eps_schedule"], grad_clipping=b["grad_clipping"])
    p = b["params_flat"].clone()
    for _ in range(3):                                  # warm: the workspace now holds p's tables (prepared calls from here on)
        mcdbm.bound_forward(seeds, p, *args, **kw)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        mcdbm.bound_forward(seeds, p, *args, **kw)      # allocator warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    c0 = dict(mcdbm.PREP_CALLS)
    with torch.cuda.graph(graph):
        l_g, z_g, s_g = mcdbm.bound_forward(seeds, p, *args, **kw)
    assert mcdbm.PREP_CALLS["full"] - c0["full"] == 1 and mcdbm.PREP_CALLS["prepared"] == c0["prepared"]
    graph.replay()
    torch.cuda.synchronize()
    l0 = l_g.clone()
    p.mul_(1.01)                                        # new parameters, same tensor
    graph.replay()
    torch.cuda.synchronize()
    l_new, _, _ = mcdbm.bound_forward(seeds, p, *args, **kw)
    assert torch.equal(l_g, l_new) and not torch.equal(l_g, l0)


@pytest.mark.parametrize("n,k", [(20, 6), (40, 3), (230, 2)])
def test_lgcp_prepared_tables(hip_lib, monkeypatch, n, k):
    """The d = 1600 sequences under cmcd_bound_forward_prepared (r04): the schedule / bias-table launches and the re-packing of
    the weights are skipped on unchanged parameters, bit-identical results; a parameter update brings them back.  20 / 40
    particles: the no-split-K passes (one, and two concurrent lanes); 230: the wide-batch form."""
    from helpers import lgcp_counts_fixture
    b = synthetic.build("lgcp_n20_k128", device="cuda", lgcp_counts=lgcp_counts_fixture(), nbridges=k, N=n, dense=True)
    seeds = torch.from_numpy(synthetic.throughput_seeds(n, stream=6)).cuda()
    args = (b["unflatten"], b["params_fixed"], b["target"])
    p = b["params_flat"].clone()
    l0, z0, s0 = mcdbm.bound_forward(seeds, p, *args)       # outside any fixed_parameters() context: a full call
    monkeypatch.setattr(mcdbm, "PREP_CACHE", True)
    was = True
    c0 = dict(mcdbm.PREP_CALLS)
    outs = [mcdbm.bound_forward(seeds, p, *args) for _ in range(4)]
    assert mcdbm.PREP_CALLS["full"] - c0["full"] == 1 and mcdbm.PREP_CALLS["prepared"] - c0["prepared"] == 3
    for l, z, st in outs:
        assert torch.equal(l, l0) and torch.equal(z, z0) and torch.equal(st, s0)
    p.mul_(1.0005)
    c1 = dict(mcdbm.PREP_CALLS)
    l1, _, s1 = mcdbm.bound_forward(seeds, p, *args)
    assert mcdbm.PREP_CALLS["full"] - c1["full"] == 1
    mcdbm.PREP_CACHE = False
    try:
        lf, _, sf = mcdbm.bound_forward(seeds, p, *args)
    finally:
        mcdbm.PREP_CACHE = was
    assert torch.equal(l1, lf) and torch.equal(s1, sf) and not torch.equal(l1, l0)


def test_prepared_tables_survive_address_reuse(hip_lib):
    with mcdbm.fixed_parameters():
        _address_reuse_body()


def test_the_shortcut_is_opt_in(hip_lib):
    """Outside `fixed_parameters()` every forward call runs its prep launch: a write that bypasses the version counter
    (`params_flat.data.mul_`) must be seen by the next call."""
    b = synthetic.build("gmm_n300_k8", device="cuda")
    seeds = torch.from_numpy(synthetic.throughput_seeds(300, stream=5)).cuda()
    args = (b["unflatten"], b["params_fixed"], b["target"])
    p = b["params_flat"].clone()
    c0 = dict(mcdbm.PREP_CALLS)
    l0 = mcdbm.bound_forward(seeds, p, *args)[0].clone()
    mcdbm.bound_forward(seeds, p, *args)
    assert mcdbm.PREP_CALLS["prepared"] == c0["prepared"] and mcdbm.PREP_CALLS["full"] - c0["full"] == 2
    v = p._version
    p.data.mul_(1.01)                                   # `.data` has its own counter: invisible to any key
    assert p._version == v
    l1 = mcdbm.bound_forward(seeds, p, *args)[0]
    assert not torch.equal(l1, l0)


def _address_reuse_body():
    """The caching allocator hands a freed tensor's address to the next tensor of the same size, and a fresh tensor's version
    counter starts where the old one's did: (address, version) does not identify a parameter tensor.  The prepared-table cache
    holds a weak reference to the tensor OBJECT; a new tensor at the old address must get a full call (r04: the sparse and the
    dense parameter set of this module collided exactly so and the second ran on the first one's tables)."""
    ba = synthetic.build("many_gmm_n2000_k256_dds", device="cuda", nbridges=8)
    bb = synthetic.build("many_gmm_n2000_k256_dds", device="cuda", nbridges=8, dense=True)
    seeds = torch.from_numpy(synthetic.throughput_seeds(512, stream=8)).cuda()
    args = (ba["unflatten"], ba["params_fixed"], ba["target"])
    kw = dict(eps_schedule=ba["eps_schedule"], grad_clipping=ba["grad_clipping"])
    host_b = bb["params_flat"].cpu()
    ref_b = mcdbm.bound_forward(seeds, bb["params_flat"], *args, **kw)[0].clone()
    pa = ba["params_flat"].clone()
    for _ in range(3):
        mcdbm.bound_forward(seeds, pa, *args, **kw)          # the workspace now holds pa's tables
    addr = pa.data_ptr()
    del pa
    reused = 0
    for _ in range(8):                                       # the allocator usually returns the block just freed
        pb = host_b.cuda()
        reused += int(pb.data_ptr() == addr)
        c0 = dict(mcdbm.PREP_CALLS)
        l = mcdbm.bound_forward(seeds, pb, *args, **kw)[0]
        assert mcdbm.PREP_CALLS["full"] - c0["full"] == 1, "a new tensor object was served another tensor's tables"
        assert torch.equal(l, ref_b)
        addr = pb.data_ptr()
        del pb
    print("address reused in", reused, "of 8 allocations")
