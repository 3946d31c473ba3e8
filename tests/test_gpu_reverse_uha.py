"""The reverse-time chain of 2nd-order CMCD (include/cmcd_hip.h: cmcd_bound_reverse_uha; cmcd_amd.reverse_uha) against the float64
NumPy restatement tests/reverse_uha_restatement.py, which tests/test_reverse_uha_oracle.py pins without a device (against the
forward oracle of the mode on its own paths).  The reference has no such call.

Parity goes through helpers.compare_losses / check_stats unchanged (w in the place of the loss, z_0 in the place of z_K); rho_0 is
held to the same z bars by a second compare_losses call.

Target draws come from exact_target_draws, as in tests/test_gpu_reverse.py.  The many_gmm cases run with init_eps = 0.05 (the
configurations' own step sizes give gamma eps > 1, tests/test_gpu_smc_uha.py).  Every parity case here, the tail case and the index
case were first run on the CPU with the restatement in float32 against the restatement in float64, and kept only because that
comparison alone stays inside the bars of compare_losses (the funnel's neck is where a leap-frog amplifies round-off): worst over
the cases rel_max 5.9e-6 (bar 1e-3; K = 64: 9.2e-6, bar 0.2), z_max / z_scale 2.6e-7 for z_0 and 2.2e-7 for rho_0 (bar 1e-3).

Seeds of the bracket test: the forward call runs on seeds 1 .. 4096 (synthetic.parity_seeds), the reverse call on seeds
100001 .. 104096 with the target draws of generator seed 11.  Verified on the CPU with the forward oracle of the mode and
`reverse_chain_uha` (float64) before they were fixed here: forward mean(-loss) = -3.4391 (se 0.0501), reverse mean(w) = +4.9552 (se 0.0703)."""
import ctypes as C
import math
import re

import numpy as np
import pytest
import torch

from cmcd_amd import _lib, reverse_uha, synthetic
from cmcd_amd import mcdboundingmachine as mcdbm
from cmcd_amd.model_handler import exact_target_draws, load_model
from helpers import check_stats, compare_losses, oracle_target
import reverse_uha_restatement as rr

MODE = "MCD_CAIS_UHA_sn"
BRACKET_N = 4096
BRACKET_REVERSE_SEED0 = 100001
BRACKET_DRAW_SEED = 11


def build(name, device="cuda", dense=True, **over):
    return synthetic.build(name, device=device, dense=dense, **dict(dict(boundmode=MODE), **over))


def target_draws(b, n, seed=5):
    cfg = b["cfg"]
    sampler = load_model(cfg["model"], None)[2]
    return exact_target_draws(cfg["model"], sampler, seed, n, b["params_fixed"][0])


def call_args(b):
    return (b["params_flat"], b["unflatten"], b["params_fixed"], b["target"]), \
        dict(eps_schedule=b["eps_schedule"], grad_clipping=b["grad_clipping"])


def run_device(b, seeds, x):
    xs = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()
    args, kw = call_args(b)
    out = reverse_uha.bound_reverse(torch.from_numpy(np.asarray(seeds, np.int32)).cuda(), xs, *args, **kw)
    torch.cuda.synchronize()
    return out


def bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def compare(tag, K, w, z0, rho0, ref):
    w_ref, z_ref, rho_ref = ref
    w, z0, rho0 = (t.cpu().numpy() for t in (w, z0, rho0))
    print(tag, "w[:4]", w[:4], "ref", w_ref[:4])
    print(tag, "z0  ", compare_losses(w, w_ref, z0, z_ref, tag, K=K))
    print(tag, "rho0", compare_losses(w, w_ref, rho0, rho_ref, tag + " (rho_0)", K=K))


# --------------------------------------------------------------------------- parity
# (id, config, overrides, n, dense): n of {1, 15, 16, 17, 33}, K of {1, 2, 8} and one funnel case at K = 64; gmm geffner 24 (T = 2),
# 44 (zero-padded to T = 4) and dds; funnel geffner 32 (T = 2), 68 (T = 5), 120 (T = 9) and dds; many_gmm geffner 134 (T = 9) and
# dds at init_eps = 0.05; the dense and the default parameter sets.
PARITY = [
    ("gmm-w24-k8-n33", "gmm_n300_k8", {}, 33, True),
    ("gmm-w24-k1-n1", "gmm_n300_k8", dict(nbridges=1), 1, False),
    ("gmm-w44-k2-n15", "gmm_n300_k8", dict(emb_dim=40, nbridges=2), 15, True),
    ("gmm-dds-k8-n16", "gmm_n300_k8", dict(nn_arch="dds"), 16, True),
    ("funnel-w32-k2-n17", "funnel_n300_k64", dict(emb_dim=12, nbridges=2), 17, True),
    ("funnel-w68-k8-n33", "funnel_n300_k64", dict(nbridges=8), 33, True),
    ("funnel-w68-k64-n16", "funnel_n300_k64", {}, 16, True),
    ("funnel-w120-k8-n15", "funnel_n300_k64", dict(emb_dim=100, nbridges=8), 15, False),
    ("funnel-dds-k8-n17", "funnel_n300_k64", dict(nn_arch="dds", nbridges=8), 17, True),
    ("many_gmm-w134-k8-n33", "many_gmm_var_n16000_k256", dict(nbridges=8, init_eps=0.05), 33, True),
    ("many_gmm-w134-k2-n16", "many_gmm_var_n16000_k256", dict(nbridges=2, init_eps=0.05), 16, False),
    ("many_gmm-dds-k8-n17", "many_gmm_n2000_k256_dds", dict(nbridges=8, init_eps=0.05), 17, True),
]


def parity_inputs(b, n):
    return synthetic.parity_seeds(n) + 40, target_draws(b, n)


@pytest.mark.gpu
@pytest.mark.parametrize("case", PARITY, ids=[c[0] for c in PARITY])
def test_parity_with_the_restatement(case):
    tag, name, over, n, dense = case
    b = build(name, dense=dense, **over)
    K = b["params_fixed"][1]
    seeds, x = parity_inputs(b, n)
    w, z0, rho0, st = run_device(b, seeds, x)
    ref = rr.run_restatement(b, seeds, x)
    compare(tag, K, w, z0, rho0, ref)
    print(tag, check_stats(st, w, tag))
    args, kw = call_args(b)
    eubo, (w2, z2) = reverse_uha.compute_reverse_bound(torch.from_numpy(seeds).cuda(), torch.from_numpy(x).cuda(), *args, **kw)
    assert abs(float(eubo) - ref[0].mean()) <= 1e-3 * max(1.0, abs(ref[0].mean()))
    assert torch.equal(bits(w2), bits(w)) and torch.equal(bits(z2), bits(z0))


# --------------------------------------------------------------------------- the clip acts
def tail_inputs(b, n=17):
    x = target_draws(b, n) + np.linspace(20.0, 160.0, n, dtype=np.float32)[:, None] * np.array([1.0, -0.9], np.float32)
    return synthetic.parity_seeds(n), x


@pytest.mark.gpu
def test_parity_far_out_in_the_tail_where_the_clip_acts():
    """x far from the mass: grad log p exceeds the clip of 1e2 (the gmm's precision x a distance of up to ~150), w spans thousands."""
    b = build("gmm_n300_k8")
    seeds, x = tail_inputs(b)
    _, gp = oracle_target(b["cfg"])(x.astype(np.float64))
    assert (np.abs(gp) > 1e2).any()
    w, z0, rho0, st = run_device(b, seeds, x)
    ref = rr.run_restatement(b, seeds, x)
    print("tail w", w.cpu().numpy())
    assert np.ptp(ref[0]) > 2e3
    compare("tail", 8, w, z0, rho0, ref)
    check_stats(st, w, "tail")


# --------------------------------------------------------------------------- the network index
def index_case(device="cuda"):
    b = build("gmm_n300_k8", device=device, nbridges=4, init_eps=0.05)
    flat = b["params_flat"].clone()
    off, shape = b["unflatten"].layout[(0, "sn", "emb")]
    flat[off:off + int(np.prod(shape))] *= 40.0          # make the bridge index count
    b = dict(b, params_flat=flat)
    n = 33
    return b, synthetic.parity_seeds(n), target_draws(b, n)


@pytest.mark.gpu
def test_both_network_evaluations_take_index_i():
    """The backward kernel of bridge i evaluates s([z_i; rho'], i) — the SAME index as the forward kernel, not i + 1 as the
    overdamped CAIS chain: a restatement with the backward evaluation at i + 1 must NOT match, on parameters where the per-bridge
    embedding matters."""
    b, seeds, x = index_case()
    w, z0, rho0, _ = run_device(b, seeds, x)
    ref = rr.run_restatement(b, seeds, x)
    compare("index", 4, w, z0, rho0, ref)
    w_bad, _, _ = rr.run_restatement(b, seeds, x, chain=rr.reverse_chain_uha_backward_at_next_index)
    assert np.abs(w_bad - ref[0]).max() > 1e-2


# --------------------------------------------------------------------------- non-finite rows
@pytest.mark.gpu
@pytest.mark.parametrize("whole_tile", [False, True])
def test_non_finite_rows_weigh_nothing(whole_tile):
    b = build("many_gmm_n2000_k256_dds", nbridges=8, init_eps=0.05)
    n = 49
    seeds = synthetic.parity_seeds(n)
    x = target_draws(b, n)
    clean_w, clean_z, clean_rho, _ = run_device(b, seeds, x)
    bad = [3, 20] + (list(range(32, 48)) if whole_tile else [])
    x = x.copy()
    x[3, 1] = np.nan
    x[20, 0] = np.inf
    for r in bad[2:]:
        x[r, r % 2] = np.nan if r % 3 else -np.inf
    w, z0, rho0, st = run_device(b, seeds, x)
    wc, good = w.cpu().numpy(), np.setdiff1d(np.arange(n), bad)
    assert np.all(wc[bad] == np.inf) and not np.isnan(wc).any()
    assert np.isfinite(wc[good]).all()
    for got, ref in ((w, clean_w), (z0, clean_z), (rho0, clean_rho)):
        assert torch.equal(bits(got[good]), bits(ref[good]))
    s = st.cpu().numpy()
    assert not np.isnan(s).any() and s[0] == n - len(bad) and s[1] == np.inf
    check_stats(st, w, "non-finite rows")
    args, kw = call_args(b)
    eubo, _ = reverse_uha.compute_reverse_bound(torch.from_numpy(seeds).cuda(), torch.from_numpy(x).cuda(), *args, **kw)
    assert float(eubo) == np.inf


# --------------------------------------------------------------------------- determinism and plumbing
@pytest.fixture(scope="module")
def funnel_case():
    b = build("funnel_n300_k64", nbridges=8)
    n = 300
    seeds = torch.from_numpy(synthetic.parity_seeds(n)).cuda()
    x = torch.from_numpy(target_draws(b, n)).cuda()
    args, kw = call_args(b)
    out = reverse_uha.bound_reverse(seeds, x, *args, **kw)
    torch.cuda.synchronize()
    return seeds, x, args, kw, out


@pytest.mark.gpu
def test_repeated_calls_give_equal_bits(funnel_case):
    seeds, x, args, kw, first = funnel_case
    again = reverse_uha.bound_reverse(seeds, x, *args, **kw)
    torch.cuda.synchronize()
    assert len(first) == 4
    for a, c in zip(first, again):
        assert torch.equal(bits(a), bits(c))


@pytest.mark.gpu
def test_a_particle_does_not_depend_on_its_batch(funnel_case):
    seeds, x, args, kw, whole = funnel_case
    rows = torch.arange(100, 117, device="cuda")       # 17 rows that straddle two tiles of the large batch
    w, z0, rho0, _ = reverse_uha.bound_reverse(seeds[rows].contiguous(), x[rows].contiguous(), *args, **kw)
    torch.cuda.synchronize()
    for got, ref in zip((w, z0, rho0), whole):
        assert torch.equal(bits(got), bits(ref[rows]))


@pytest.mark.gpu
def test_graph_capture_and_replay(funnel_case):
    seeds, x, args, kw, eager = funnel_case
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        reverse_uha.bound_reverse(seeds, x, *args, **kw)      # allocator warm-up on a side stream
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = reverse_uha.bound_reverse(seeds, x, *args, **kw)
    for t in captured:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for a, c in zip(eager, captured):
        assert torch.equal(bits(a), bits(c))


@pytest.mark.gpu
def test_non_default_stream(funnel_case):
    seeds, x, args, kw, eager = funnel_case
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out = reverse_uha.bound_reverse(seeds, x, *args, **kw)
    side.synchronize()
    for a, c in zip(eager, out):
        assert torch.equal(bits(a), bits(c))


# --------------------------------------------------------------------------- the bracket
def bracket_reverse_inputs(b):
    n = BRACKET_N
    return np.arange(BRACKET_REVERSE_SEED0, BRACKET_REVERSE_SEED0 + n, dtype=np.int32), target_draws(b, n, seed=BRACKET_DRAW_SEED)


@pytest.mark.gpu
def test_elbo_and_eubo_bracket_ln_z():
    """gmm is normalised (ln Z = 0): E_Q[-loss] <= 0 <= E_P[w], each within 4 standard errors of its own sample."""
    b = build("gmm_n300_k8")
    n = BRACKET_N
    args, kw = call_args(b)
    loss, _, _ = mcdbm.bound_forward(torch.from_numpy(synthetic.parity_seeds(n)).cuda(), *args, **kw)
    seeds, x = bracket_reverse_inputs(b)
    w, _, _, st = reverse_uha.bound_reverse(torch.from_numpy(seeds).cuda(), torch.from_numpy(x).cuda(), *args, **kw)
    torch.cuda.synchronize()
    f, r = -loss.double().cpu().numpy(), w.double().cpu().numpy()
    se_f, se_r = f.std(ddof=1) / np.sqrt(n), r.std(ddof=1) / np.sqrt(n)
    print("forward mean(-loss) %.4f (se %.4f); reverse mean(w) %.4f (se %.4f); reverse ln Z %.4f" % (
        f.mean(), se_f, r.mean(), se_r, -float(mcdbm.ln_z_from_stats(st, n))))
    assert np.isfinite(f).all() and np.isfinite(r).all()
    assert f.mean() <= 0.0 + 4 * se_f
    assert r.mean() >= 0.0 - 4 * se_r


# --------------------------------------------------------------------------- refusals
@pytest.mark.gpu
def test_unsupported_configurations_raise():
    n = 32
    seeds = torch.arange(1, n + 1, dtype=torch.int32, device="cuda")
    x = torch.zeros((n, 2), device="cuda")
    for mode in ("MCD_CAIS_sn", "MCD_CAIS_var_sn", "MCD_ULA", "MCD_ULA_sn"):      # the overdamped modes: mcdbm.bound_reverse's
        b = build("gmm_n300_k8", boundmode=mode, dense=False)
        with pytest.raises(NotImplementedError, match="cmcd_bound_reverse"):
            reverse_uha.bound_reverse(seeds, x, *call_args(b)[0])
    b = build("gmm_n300_k8", emb_dim=198, dense=False)                             # width 202: no instance
    with pytest.raises(NotImplementedError):
        reverse_uha.bound_reverse(seeds, x, *call_args(b)[0])
    from helpers import lgcp_counts_fixture
    b = build("lgcp_n20_k128", lgcp_counts=lgcp_counts_fixture(), nbridges=2, dense=False)
    with pytest.raises(NotImplementedError, match="lgcp"):
        reverse_uha.bound_reverse(seeds, torch.zeros((n, 1600), device="cuda"), *call_args(b)[0])


@pytest.mark.gpu
def test_bad_inputs_fail_before_any_launch():
    b = build("gmm_n300_k8", dense=False)
    n = 32
    seeds = torch.arange(1, n + 1, dtype=torch.int32, device="cuda")
    args = call_args(b)[0]
    good = torch.zeros((n, 2), device="cuda")
    with pytest.raises(RuntimeError, match="ROCm device"):
        reverse_uha.bound_reverse(seeds, good.cpu(), *args)
    with pytest.raises(ValueError, match="shape"):
        reverse_uha.bound_reverse(seeds, torch.zeros((n, 3), device="cuda"), *args)
    with pytest.raises(ValueError, match="shape"):
        reverse_uha.bound_reverse(seeds, torch.zeros((n + 1, 2), device="cuda"), *args)
    with pytest.raises(ValueError, match="float32"):
        reverse_uha.bound_reverse(seeds, good.double(), *args)
    with pytest.raises(ValueError, match="contiguous"):
        reverse_uha.bound_reverse(seeds, torch.zeros((2, n), device="cuda").t(), *args)
    # the C level: a workspace one byte short, a null x
    L = _lib.lib()
    plan = mcdbm._plan(b["unflatten"], b["params_fixed"], b["target"], b["eps_schedule"], b["grad_clipping"])
    need = L.cmcd_reverse_uha_workspace_bytes(C.byref(plan.desc), n)
    assert need > 0 and need == L.cmcd_workspace_bytes(C.byref(plan.desc), n)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    w, z0, st = mcdbm._outputs(n, 2, good.device)
    rho0 = torch.empty_like(z0)
    w.fill_(7.0)

    def call(x_ptr, ws_bytes):
        return L.cmcd_bound_reverse_uha(C.byref(plan.desc), C.byref(plan.lay), seeds.data_ptr(), x_ptr, n, b["params_flat"].data_ptr(),
                                        b["params_flat"].numel(), None, 0, ws.data_ptr(), ws_bytes, w.data_ptr(), z0.data_ptr(),
                                        rho0.data_ptr(), st.data_ptr(), None)

    assert call(good.data_ptr(), need - 1) == -3 and "workspace too small" in _lib.last_error()
    assert call(None, need) == -1 and "null pointer" in _lib.last_error()
    torch.cuda.synchronize()
    assert bool((w == 7.0).all())                 # nothing ran
    assert call(good.data_ptr(), need) == 0
    torch.cuda.synchronize()
    assert bool((w != 7.0).all())


# --------------------------------------------------------------------------- the driver
DRIVER_ARGV = ["--config.model", "gmm", "--config.boundmode", MODE, "--config.N", "16", "--config.nbridges", "4",
               "--config.mfvi_iters", "20", "--config.iters", "20", "--config.n_samples", "32", "--config.n_input_dist_seeds", "3",
               "--config.init_eps", "0.01", "--config.lr", "0.001", "--noconfig.compute_w2"]


@pytest.mark.gpu
def test_driver_prints_the_reverse_chain_line_for_this_boundmode(hip_lib, capsys):
    from cmcd_amd import main as cli
    elbo, ln_z = cli.main(cli.parse_flags(DRIVER_ARGV, cli.get_config()))
    out = capsys.readouterr().out
    assert math.isfinite(elbo) and math.isfinite(ln_z)
    m = re.search(r"Reverse chain: EUBO (\S+), reverse ln Z (\S+), reverse ESS (\S+) \(", out)
    assert m, out
    assert all(math.isfinite(float(v)) for v in m.groups()), m.groups()
    assert out.count("Reverse chain") == 1


@pytest.mark.gpu
def test_driver_skips_the_reverse_chain_on_request(hip_lib, capsys):
    from cmcd_amd import main as cli
    elbo, ln_z = cli.main(cli.parse_flags(DRIVER_ARGV + ["--noconfig.compute_eubo"], cli.get_config()))
    out = capsys.readouterr().out
    assert math.isfinite(elbo) and math.isfinite(ln_z)
    assert "Reverse chain" not in out
