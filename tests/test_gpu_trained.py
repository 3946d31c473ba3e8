"""The HIP path against the float64 oracle where training takes the parameters (tests/trained_cases.py): snapshots of trained
runs — grown networks, a beta grid far from uniform, a learnt q — and the faces of the projection box (eps = 1e-7 and 0.5,
gamma = 1e-3, mgridref_y entries at 1e-3).  tests/test_oracle_trained_params.py asserts on the CPU what each case is.

Forward: every kernel form the case can run, all three outputs through helpers.compare_losses; the reverse chain and a split
segment chain for the overdamped snapshots.  Gradients: every path of tests/test_gpu_grad.py / test_gpu_uha.py / test_gpu_hais.py,
leaf by leaf through test_gpu_grad._compare.

Bars (trained_cases.loss_bars / grad_tols): the suite's standard ones — compare_losses' defaults, 2e-3 per leaf — wherever the
float32 gap of the oracle itself (LOSS_GAP32 / GRAD_GAP32) is at most a quarter of the bar; otherwise four times that gap (other
summation orders, fused multiply-adds and the kernels' log2-domain target arithmetic should not cost more than the restatement's
own rounding does).  The cases on a loosened bar are the eps = 1e-7 ones and a few leaves next to them: DESIGN.md section 2.
Every run prints what it observed before it asserts."""
import functools

import numpy as np
import pytest
import torch

import trained_cases as tc
from cmcd_amd import mcdboundingmachine as mcdbm
from helpers import compare_losses

pytestmark = pytest.mark.gpu

_UHA_SN = "MCD_CAIS_UHA_sn"
OVERDAMPED = ("MCD_CAIS_sn", "MCD_CAIS_var_sn", "MCD_ULA_sn", "MCD_ULA")


def dim_of(case):
    model = tc.TRAINED_ROWS[case[0]]["model"] if tc.is_trained(case) else case[1]
    return 10 if "funnel" in model else 2


def forward_variants(case):
    """KERNEL_VARIANT values as tests/test_gpu_parity.py / test_gpu_uha.py run them (None: the call has no forms)."""
    mode = case[4]
    if mode == "UHA":
        return [None]
    if mode == _UHA_SN:
        return [1, 3, 4]
    if mode == "MCD_ULA":
        return [1]                                     # no network: the cooperative (MLP-split) kernels do not apply
    return [1, 3, 4, 5] if dim_of(case) == 10 else [1, 2, 3]


def gradient_paths(case):
    """(KERNEL_VARIANT, CMCD_GRAD_ITEM) pairs as the gradient tests of each mode run them."""
    return {"MCD_CAIS_sn": [(1, 0), (2, 0), (1, 1), (2, 1), (3, 1)], "MCD_CAIS_var_sn": [(None, 0), (None, 1)],
            "MCD_ULA_sn": [(1, 0), (2, 1), (1, 1)], "MCD_ULA": [(None, None)], _UHA_SN: [(1, 0), (3, 0), (4, 0), (3, 1)],
            "UHA": [(None, None)]}[case[4]]


@functools.lru_cache(maxsize=None)
def hais_target(name):
    from cmcd_amd import model_handler
    return model_handler.load_model(name)[0]


@functools.lru_cache(maxsize=None)
def forward_reference(cid):
    """(losses, z) of the float64 oracle on the case's seeds: computed once, shared, never written to."""
    case = tc.case_by_id(cid)
    return tc.forward_oracle(tc.build_case(case), case[3])


@functools.lru_cache(maxsize=None)
def gradient_reference(cid):
    """(losses, z, flat gradient) of the float64 autograd oracle on the case as its gradient comparisons run it."""
    case = tc.case_by_id(cid)
    return tc.grad_oracle(tc.build_case(case, grad=True), case[3])


def dev(seeds):
    return torch.from_numpy(np.asarray(seeds, np.int32)).cuda()


def skip_without_cooperative_instance(call):
    try:
        return call()
    except NotImplementedError as e:
        if "cooperative" in str(e):
            pytest.skip("no cooperative instance for this net")
        raise


def assert_losses(case, l, z, l_ref, z_ref, tag, K=None):
    """compare_losses under the case's bars; prints the observed metrics first."""
    K = tc.bridges_of(case) if K is None else K
    obs, z_scale = tc.loss_metrics(l, l_ref, z, z_ref)
    bars, std = tc.loss_bars(case[0], K), tc.standard_loss_bars(K)
    print("OBSERVED", tag, {k: "%.2e" % v for k, v in obs.items()}, "bars", {k: v for k, v in bars.items() if v != std[k]})
    loose = {k: bars[k] for k in ("mean", "lnz", "rel_p99", "z_p99") if bars[k] != std[k]}
    return compare_losses(l, l_ref, z, z_ref, tag=tag, K=K, rel_max=bars["rel_max"] if bars["rel_max"] != std["rel_max"] else None,
                          z_max=bars["z_max"] * z_scale if bars["z_max"] != std["z_max"] else None, bars=loose or None)


_FWD_RUNS = [pytest.param(c, v, id=f"{c[0]}-variant{v}") for c in tc.CASES for v in forward_variants(c)]


@pytest.mark.parametrize("case,variant", _FWD_RUNS)
def test_forward_matches_the_oracle(hip_lib, monkeypatch, case, variant):
    if variant is not None:
        monkeypatch.setattr(mcdbm, "KERNEL_VARIANT", variant)
    b = tc.build_case(case, device="cuda")
    l_ref, z_ref = forward_reference(case[0])
    if b["kind"] == "hais":
        from cmcd_amd import hais
        val, (losses, z) = hais.compute_bound(dev(case[3]), b["params_flat"], b["unflatten"], b["params_fixed"],
                                              hais_target(b["target_name"]))
    else:
        fn = mcdbm.compute_bound_var if case[4] == "MCD_CAIS_var_sn" else mcdbm.compute_bound
        val, (losses, z) = skip_without_cooperative_instance(lambda: fn(
            dev(case[3]), b["params_flat"], b["unflatten"], b["params_fixed"], b["target"], eps_schedule=b["eps_schedule"],
            grad_clipping=b["grad_clipping"]))
    torch.cuda.synchronize()
    assert_losses(case, losses.cpu().numpy(), z.cpu().numpy(), l_ref, z_ref, f"forward {case[0]} variant {variant}")
    lh = losses.double().cpu().numpy()
    want = np.clip(np.var(lh), -1e7, 1e7) if case[4] == "MCD_CAIS_var_sn" else np.mean(lh)
    if np.isfinite(want):
        assert abs(float(val) - want) <= 1e-5 * max(1.0, abs(want))
    else:
        assert not np.isfinite(float(val))


_SNAPSHOTS = [c for c in tc.CASES if tc.is_trained(c) and c[4] in OVERDAMPED]


@pytest.mark.parametrize("case", _SNAPSHOTS, ids=[c[0] for c in _SNAPSHOTS])
def test_reverse_chain_on_a_trained_snapshot(hip_lib, case):
    """cmcd_bound_reverse reads the same prepared tables as the forward call and has its own chain code."""
    from test_gpu_reverse import run_device, run_restatement, target_draws
    b = tc.build_case(case, device="cuda")
    seeds = np.asarray(case[3], np.int32)
    x = target_draws(b, len(seeds))
    w, z0, _ = run_device(b, seeds, x)
    w_ref, z_ref = run_restatement(b, seeds, x)
    K = tc.bridges_of(case)
    print("OBSERVED reverse", case[0], compare_losses(w.cpu().numpy(), w_ref, z0.cpu().numpy(), z_ref, f"reverse {case[0]}", K=K))


@pytest.mark.parametrize("case", _SNAPSHOTS, ids=[c[0] for c in _SNAPSHOTS])
def test_split_segment_chain_on_a_trained_snapshot(hip_lib, case):
    """smc.segment over [0, K / 2) and, from the state that call left on the device, [K / 2, K): against the float64
    restatement of the whole chain."""
    import smc_restatement as rs
    from cmcd_amd import smc
    b = tc.build_case(case, device="cuda")
    K = tc.bridges_of(case)
    args = (b["params_flat"], b["unflatten"], b["params_fixed"], b["target"], b["eps_schedule"], b["grad_clipping"])
    head = smc.segment(dev(case[3]), 0, K // 2, *args)
    out = smc.segment(head, K // 2, K, *args)
    torch.cuda.synchronize()
    ref = rs.segment_runner(b)(np.asarray(case[3], np.int32), 0, K)
    assert np.array_equal(out["key"].cpu().numpy().view(np.uint32), ref["key"])
    print("OBSERVED segment", case[0], compare_losses(smc.losses_of(out).cpu().numpy(), rs.losses_of(ref), out["z"].cpu().numpy(),
                                                      ref["z"], f"segment {case[0]}", K=K))


_GRAD_RUNS = [pytest.param(c, v, i, id=f"{c[0]}-variant{v}-item{i}") for c in tc.CASES for v, i in gradient_paths(c)]


@pytest.mark.parametrize("case,variant,item", _GRAD_RUNS)
def test_gradient_matches_autograd(hip_lib, monkeypatch, case, variant, item):
    from test_gpu_grad import _compare, compare_losses_with_inf
    if variant is not None:
        monkeypatch.setattr(mcdbm, "KERNEL_VARIANT", variant)
    if item is not None:
        monkeypatch.setenv("CMCD_GRAD_ITEM", str(item))
    b = tc.build_case(case, device="cuda", grad=True)
    l_ref, z_ref, g_ref = gradient_reference(case[0])
    if b["kind"] == "hais":
        from cmcd_amd import hais
        grad, (losses, z) = hais.grad_and_loss(dev(case[3]), b["params_flat"], b["unflatten"], b["params_fixed"],
                                               hais_target(b["target_name"]))
    else:
        fn = mcdbm.compute_log_var_grad if case[4] == "MCD_CAIS_var_sn" else mcdbm.compute_bound_grad
        grad, (losses, z) = skip_without_cooperative_instance(lambda: fn(
            dev(case[3]), b["params_flat"], b["unflatten"], b["params_fixed"], b["target"], eps_schedule=b["eps_schedule"],
            grad_clipping=b["grad_clipping"]))
    torch.cuda.synchronize()
    g = grad.double().cpu()
    tols = tc.grad_tols(case[0])
    print("OBSERVED gradient", case[0], variant, item, {k: "%.2e" % v for k, v in tc.leaf_errors(b["unflatten"], g, g_ref).items()},
          "bars", tols)
    compare_losses_with_inf(losses.cpu().numpy(), l_ref)
    assert bool(torch.isfinite(grad).all())
    _compare(case[0], case[2], b["unflatten"], g, g_ref, tol=tols or 2e-3)
