"""The reverse-time chain of LDVI (include/cmcd_hip.h: cmcd_bound_reverse_ldvi; cmcd_amd.reverse_ldvi) against the float64 NumPy
restatement tests/reverse_ldvi_restatement.py, which tests/test_reverse_ldvi_oracle.py pins without a device (against the forward
restatement of the mode on its own paths).  The reference has no such call.

Parity goes through helpers.compare_losses / check_stats unchanged (w in the place of the loss, z_0 in the place of z_K); rho_0 is
held to the same z bars by a second compare_losses call.  Every case is the dense parameter set except the one-particle case.

Target draws come from exact_target_draws.  The funnel cases run at tests/ldvi_cases.py's step sizes (eps 0.05, gamma 4; K = 64:
eps 0.01), the many_gmm cases at init_eps = 0.05, init_gamma = 2.0.  Every parity case here and the wrong-chain case were first run
on the CPU with the restatement in float32 against the restatement in float64, and kept only because that comparison
alone stays inside the default bars of compare_losses: worst over the cases rel_max 1.1e-5 (bar 1e-3; K = 64: 8.4e-6, bar 0.2),
z_max / z_scale 4.3e-7 for z_0 and 4.0e-7 for rho_0 (bar 1e-3).  On the float64 restatement no row of a many_gmm case has an evaluation
within ldvi_cases.BAND (500) of the floor: the guard drops no row (closest: 9.99e3 above the floor, log p >= -8.1 at every state).

Seeds of the bracket test: the forward call runs on seeds 1 .. 4096 (synthetic.parity_seeds), the reverse call on seeds
100001 .. 104096 with the target draws of generator seed 11.  Verified on the CPU with the float64 restatements before they were
fixed here: forward mean(-loss) = -3.4320 (se 0.0499), reverse mean(w) = +4.9590 (se 0.0704) (BRACKET_FORWARD / BRACKET_REVERSE)."""
import ctypes as C
import functools
import math
import re

import numpy as np
import pytest
import torch

import ldvi_restatement as lr
import reverse_ldvi_restatement as rl
from cmcd_amd import _lib, ldvi, reverse_ldvi, synthetic
from cmcd_amd.model_handler import exact_target_draws, load_model
from helpers import check_stats, compare_losses
from test_reverse_ldvi_oracle import gpu_wrong_chain_case, wrong_chain_inputs

SN, PLAIN = "MCD_U_a-lp-sn", "MCD_U_a-lp"
BRACKET_N = 4096
BRACKET_REVERSE_SEED0 = 100001
BRACKET_DRAW_SEED = 11
# float64 restatements on the bracket's inputs (CPU): mean and standard error
BRACKET_FORWARD = (-3.4320, 0.0499)      # mean(-loss) of ldvi_restatement.forward on seeds 1 .. 4096: 68 standard errors below 0
BRACKET_REVERSE = (+4.9590, 0.0704)      # mean(w) of reverse_chain_ldvi: 70 standard errors above 0

_FUNNEL = dict(init_eps=0.05, init_gamma=4.0)
_MANY = dict(nn_arch="geffner", emb_dim=20, init_eps=0.05, init_gamma=2.0)


def build(name, mode=SN, device="cuda", dense=True, **over):
    b = synthetic.build(name, device=device, dense=dense, boundmode="MCD_CAIS_UHA_sn" if mode == SN else "MCD_ULA", **over)
    dim, K, _, spec = b["params_fixed"]
    b["params_fixed"] = (dim, K, mode, spec)
    return b


def target_draws(b, n, seed=5):
    cfg = b["cfg"]
    sampler = load_model(cfg["model"], None)[2]
    return exact_target_draws(cfg["model"], sampler, seed, n, b["params_fixed"][0])


def call_args(b):
    return (b["params_flat"], b["unflatten"], b["params_fixed"], b["target"])


def run_device(b, seeds, x):
    xs = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()
    out = reverse_ldvi.bound_reverse(torch.from_numpy(np.asarray(seeds, np.int32)).cuda(), xs, *call_args(b))
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
# (id, config, mode, overrides, n, dense)
PARITY = [
    ("gmm-w24-k8-n33", "gmm_n300_k8", SN, {}, 33, True),
    ("gmm-w24-k1-n1", "gmm_n300_k8", SN, dict(nbridges=1), 1, False),
    ("gmm-w44-k2-n15", "gmm_n300_k8", SN, dict(emb_dim=40, nbridges=2), 15, True),
    ("gmm-w64-k8-n16", "gmm_n300_k8", SN, dict(emb_dim=60), 16, True),
    ("funnel-w68-k8-n17", "funnel_n300_k64", SN, dict(_FUNNEL, nbridges=8), 17, True),
    ("funnel-w80-k2-n16", "funnel_n300_k64", SN, dict(_FUNNEL, emb_dim=60, nbridges=2), 16, True),
    ("funnel-w68-k64-n16", "funnel_n300_k64", SN, dict(init_eps=0.01, init_gamma=4.0), 16, True),
    ("many_gmm-w24-k8-n33", "many_gmm_n2000_k256_dds", SN, dict(_MANY, nbridges=8), 33, True),
    ("many_gmm-w64-k2-n17", "many_gmm_n2000_k256_dds", SN, dict(_MANY, emb_dim=60, nbridges=2), 17, True),
    ("nonet-gmm-n33", "gmm_n300_k8", PLAIN, {}, 33, True),
    ("nonet-funnel-n17", "funnel_n300_k64", PLAIN, dict(_FUNNEL, nbridges=8), 17, True),
    ("nonet-many_gmm-n17", "many_gmm_n2000_k256_dds", PLAIN, dict(_MANY, nbridges=8), 17, True),
    # the launch rule: 1025 tiles = 4 waves per workgroup, the last with one live wave; 8193 tiles = 8 waves per workgroup
    ("gmm-nw4-k1-n16400", "gmm_n300_k8", SN, dict(nbridges=1), 16400, True),
    ("gmm-nw8-k1-n131088", "gmm_n300_k8", SN, dict(nbridges=1), 131088, True),
]


def parity_inputs(b, n):
    return synthetic.parity_seeds(n) + 40, target_draws(b, n)


@pytest.mark.gpu
@pytest.mark.parametrize("case", PARITY, ids=[c[0] for c in PARITY])
def test_parity_with_the_restatement(case):
    tag, name, mode, over, n, dense = case
    b = build(name, mode, dense=dense, **over)
    K = b["params_fixed"][1]
    seeds, x = parity_inputs(b, n)
    w, z0, rho0, st = run_device(b, seeds, x)
    ref = rl.run_restatement(b, seeds, x)
    compare(tag, K, w, z0, rho0, ref)
    print(tag, check_stats(st, w, tag))
    eubo, (w2, z2) = reverse_ldvi.compute_reverse_bound(torch.from_numpy(seeds).cuda(), torch.from_numpy(x).cuda(), *call_args(b))
    assert abs(float(eubo) - ref[0].mean()) <= 1e-3 * max(1.0, abs(ref[0].mean()))
    assert torch.equal(bits(w2), bits(w)) and torch.equal(bits(z2), bits(z0))


# --------------------------------------------------------------------------- the wrong chains
@pytest.mark.gpu
def test_the_device_is_held_apart_from_each_wrong_chain():
    """The backward network takes index i (not i + 1), and the forward mean has NO network (not 2nd-order CMCD's): the device matches
    the right restatement on parameters where both matter, and each wrong chain is more than 100 bars away from it
    (tests/test_reverse_ldvi_oracle.py measures 0.26 and 0.27 against the bar of 1e-3)."""
    b = gpu_wrong_chain_case(device="cuda")
    seeds, x = wrong_chain_inputs(b)
    w, z0, rho0, _ = run_device(b, seeds, x)
    ref = rl.run_restatement(b, seeds, x)
    compare("wrong-chain case", 4, w, z0, rho0, ref)
    wd = w.double().cpu().numpy()
    for chain in (rl.reverse_chain_ldvi_backward_at_next_index, rl.reverse_chain_ldvi_forward_mean_with_network):
        w_bad, _, _ = rl.run_restatement(b, seeds, x, chain=chain)
        assert (np.abs(w_bad - wd) / np.maximum(1.0, np.abs(wd))).max() > 0.1, chain.__name__


# --------------------------------------------------------------------------- non-finite rows
@pytest.mark.gpu
@pytest.mark.parametrize("whole_tile", [False, True])
def test_non_finite_rows_weigh_nothing(whole_tile):
    b = build("many_gmm_n2000_k256_dds", **dict(_MANY, nbridges=8))
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
    eubo, _ = reverse_ldvi.compute_reverse_bound(torch.from_numpy(seeds).cuda(), torch.from_numpy(x).cuda(), *call_args(b))
    assert float(eubo) == np.inf


@pytest.mark.gpu
def test_a_draw_under_the_floor_of_many_gmm_weighs_nothing():
    b = build("many_gmm_n2000_k256_dds", **dict(_MANY, nbridges=2))
    n = 17
    seeds = synthetic.parity_seeds(n)
    x = target_draws(b, n).copy()
    x[5] = (400.0, -400.0)          # log p far under -1e4
    w, z0, rho0, st = run_device(b, seeds, x)
    ref = rl.run_restatement(b, seeds, x)
    assert ref[0][5] == np.inf and float(w[5]) == np.inf
    compare("floored draw", 2, w, z0, rho0, ref)
    check_stats(st, w, "floored draw")


# --------------------------------------------------------------------------- determinism and plumbing
@pytest.fixture(scope="module")
def funnel_case():
    b = build("funnel_n300_k64", **dict(_FUNNEL, nbridges=8))
    n = 300
    seeds = torch.from_numpy(synthetic.parity_seeds(n)).cuda()
    x = torch.from_numpy(target_draws(b, n)).cuda()
    args = call_args(b)
    out = reverse_ldvi.bound_reverse(seeds, x, *args)
    torch.cuda.synchronize()
    return seeds, x, args, out


@pytest.mark.gpu
def test_repeated_calls_give_equal_bits(funnel_case):
    seeds, x, args, first = funnel_case
    again = reverse_ldvi.bound_reverse(seeds, x, *args)
    torch.cuda.synchronize()
    assert len(first) == 4
    for a, c in zip(first, again):
        assert torch.equal(bits(a), bits(c))


@pytest.mark.gpu
def test_a_particle_does_not_depend_on_its_batch(funnel_case):
    seeds, x, args, whole = funnel_case
    rows = torch.arange(100, 117, device="cuda")       # 17 rows that straddle two tiles of the large batch
    w, z0, rho0, _ = reverse_ldvi.bound_reverse(seeds[rows].contiguous(), x[rows].contiguous(), *args)
    torch.cuda.synchronize()
    for got, ref in zip((w, z0, rho0), whole):
        assert torch.equal(bits(got), bits(ref[rows]))


@pytest.mark.gpu
def test_graph_capture_and_replay(funnel_case):
    seeds, x, args, eager = funnel_case
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        reverse_ldvi.bound_reverse(seeds, x, *args)      # allocator warm-up on a side stream
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = reverse_ldvi.bound_reverse(seeds, x, *args)
    for t in captured:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for a, c in zip(eager, captured):
        assert torch.equal(bits(a), bits(c))


@pytest.mark.gpu
def test_non_default_stream(funnel_case):
    seeds, x, args, eager = funnel_case
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out = reverse_ldvi.bound_reverse(seeds, x, *args)
    side.synchronize()
    for a, c in zip(eager, out):
        assert torch.equal(bits(a), bits(c))


# --------------------------------------------------------------------------- the bracket
def bracket_reverse_inputs(b):
    n = BRACKET_N
    return np.arange(BRACKET_REVERSE_SEED0, BRACKET_REVERSE_SEED0 + n, dtype=np.int32), target_draws(b, n, seed=BRACKET_DRAW_SEED)


@functools.lru_cache(maxsize=None)
def bracket_reference():
    """The float64 restatements on the bracket's inputs -> (-loss[N], w[N])."""
    b = build("gmm_n300_k8", device="cpu")
    dim, K, _, _ = b["params_fixed"]
    loss, _ = lr.forward(synthetic.parity_seeds(BRACKET_N), lr.params_numpy(b["unflatten"], b["params_flat"]), dim, K, "gmm")
    seeds, x = bracket_reverse_inputs(b)
    return -loss, rl.run_restatement(b, seeds, x)[0]


@pytest.mark.gpu
def test_elbo_and_eubo_bracket_ln_z():
    """gmm is normalised (ln Z = 0): E_Q[-loss] < 0 < E_P[w]; on the float64 restatements each mean lies more than 5 of its standard
    errors away from 0 (BRACKET_FORWARD, BRACKET_REVERSE), and the device's means are within 1e-3 max(1, |ref|) of them."""
    b = build("gmm_n300_k8")
    n = BRACKET_N
    args = call_args(b)
    loss, _, _ = ldvi.bound_forward(torch.from_numpy(synthetic.parity_seeds(n)).cuda(), *args)
    seeds, x = bracket_reverse_inputs(b)
    w, _, _, st = reverse_ldvi.bound_reverse(torch.from_numpy(seeds).cuda(), torch.from_numpy(x).cuda(), *args)
    torch.cuda.synchronize()
    f, r = -loss.double().cpu().numpy(), w.double().cpu().numpy()
    f_ref, r_ref = bracket_reference()
    for name, got, ref, recorded in (("forward", f, f_ref, BRACKET_FORWARD), ("reverse", r, r_ref, BRACKET_REVERSE)):
        se = ref.std(ddof=1) / np.sqrt(n)
        print("%s: device mean %.4f; restatement mean %.4f (se %.4f)" % (name, got.mean(), ref.mean(), se))
        assert abs(ref.mean() - recorded[0]) < 1e-3 and abs(se - recorded[1]) < 1e-3      # the recorded figures are the restatement's
        assert abs(ref.mean()) > 5 * se
        assert np.isfinite(got).all()
        assert abs(got.mean() - ref.mean()) <= 1e-3 * max(1.0, abs(ref.mean()))
    assert f.mean() < 0.0 < r.mean()


# --------------------------------------------------------------------------- refusals
@pytest.mark.gpu
def test_unsupported_configurations_raise():
    n = 32
    seeds = torch.arange(1, n + 1, dtype=torch.int32, device="cuda")
    x = torch.zeros((n, 2), device="cuda")
    b = build("gmm_n300_k8", emb_dim=130, dense=False)                             # width 134: 9 tiles, no LDVI instance
    with pytest.raises(NotImplementedError, match="kernel instance"):
        reverse_ldvi.bound_reverse(seeds, x, *call_args(b))
    b = build("funnel_n300_k64", emb_dim=12, nbridges=2, dense=False)              # the funnel on 2 tiles
    with pytest.raises(NotImplementedError, match="kernel instance"):
        reverse_ldvi.bound_reverse(seeds, torch.zeros((n, 10), device="cuda"), *call_args(b))
    b = build("gmm_n300_k8", nn_arch="dds", dense=False)
    with pytest.raises(NotImplementedError, match="dds"):
        reverse_ldvi.bound_reverse(seeds, x, *call_args(b))
    for mode in ("MCD_CAIS_UHA_sn", "MCD_CAIS_sn"):                                # not an LDVI mode string
        b = synthetic.build("gmm_n300_k8", device="cuda", boundmode=mode)
        with pytest.raises(NotImplementedError, match="Mode not implemented"):
            reverse_ldvi.bound_reverse(seeds, x, *call_args(b))
    # ... and the 2nd-order module keeps refusing the LDVI mode strings
    from cmcd_amd import reverse_uha
    b = build("gmm_n300_k8", dense=False)
    with pytest.raises(NotImplementedError, match="Mode not implemented"):
        reverse_uha.bound_reverse(seeds, x, *call_args(b))


@pytest.mark.gpu
def test_bad_inputs_fail_before_any_launch():
    b = build("gmm_n300_k8", dense=False)
    n = 32
    seeds = torch.arange(1, n + 1, dtype=torch.int32, device="cuda")
    args = call_args(b)
    good = torch.zeros((n, 2), device="cuda")
    with pytest.raises(RuntimeError, match="ROCm device"):
        reverse_ldvi.bound_reverse(seeds, good.cpu(), *args)
    with pytest.raises(ValueError, match="shape"):
        reverse_ldvi.bound_reverse(seeds, torch.zeros((n, 3), device="cuda"), *args)
    with pytest.raises(ValueError, match="shape"):
        reverse_ldvi.bound_reverse(seeds, torch.zeros((n + 1, 2), device="cuda"), *args)
    with pytest.raises(ValueError, match="float32"):
        reverse_ldvi.bound_reverse(seeds, good.double(), *args)
    with pytest.raises(ValueError, match="contiguous"):
        reverse_ldvi.bound_reverse(seeds, torch.zeros((2, n), device="cuda").t(), *args)
    # the C level: a workspace one byte short, a null x
    L = _lib.lib()
    desc, lay, use_net = ldvi._plan(b["unflatten"], b["params_fixed"], b["target"])
    need = L.cmcd_reverse_ldvi_workspace_bytes(C.byref(desc), use_net, n)
    assert need > 0 and need == L.cmcd_ldvi_workspace_bytes(C.byref(desc), use_net, n, 0)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    from cmcd_amd import mcdboundingmachine as mcdbm
    w, z0, st = mcdbm._outputs(n, 2, good.device)
    rho0 = torch.empty_like(z0)
    w.fill_(7.0)

    def call(x_ptr, ws_bytes):
        return L.cmcd_bound_reverse_ldvi(C.byref(desc), C.byref(lay), use_net, seeds.data_ptr(), x_ptr, n, b["params_flat"].data_ptr(),
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
DRIVER_ARGV = ["--config.model", "gmm", "--config.N", "16", "--config.nbridges", "4",
               "--config.mfvi_iters", "20", "--config.iters", "20", "--config.n_samples", "32", "--config.n_input_dist_seeds", "3",
               "--config.init_eps", "0.01", "--config.lr", "0.001", "--noconfig.compute_w2"]


@pytest.mark.gpu
@pytest.mark.parametrize("boundmode", [SN, PLAIN])
def test_driver_prints_the_reverse_chain_line_for_the_ldvi_modes(hip_lib, capsys, boundmode):
    from cmcd_amd import main as cli
    elbo, ln_z = cli.main(cli.parse_flags(DRIVER_ARGV + ["--config.boundmode", boundmode], cli.get_config()))
    out = capsys.readouterr().out
    assert math.isfinite(elbo) and math.isfinite(ln_z)
    m = re.search(r"Reverse chain: EUBO (\S+), reverse ln Z (\S+), reverse ESS (\S+) \(", out)
    assert m, out
    assert all(math.isfinite(float(v)) for v in m.groups()), m.groups()
    assert out.count("Reverse chain") == 1


@pytest.mark.gpu
def test_driver_skips_the_reverse_chain_on_request(hip_lib, capsys):
    from cmcd_amd import main as cli
    elbo, ln_z = cli.main(cli.parse_flags(DRIVER_ARGV + ["--config.boundmode", SN, "--noconfig.compute_eubo"], cli.get_config()))
    out = capsys.readouterr().out
    assert math.isfinite(elbo) and math.isfinite(ln_z)
    assert "Reverse chain" not in out
