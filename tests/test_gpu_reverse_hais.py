"""The reverse-time chain of UHA, Hamiltonian AIS (include/cmcd_hip.h: cmcd_bound_reverse_hais; cmcd_amd.reverse_hais) against the
float64 NumPy restatement tests/reverse_hais_restatement.py, which tests/test_reverse_hais_oracle.py pins without a device (against
the forward restatement of the mode on its own paths).  The reference has no such call.

Parity goes through helpers.compare_losses / check_stats unchanged (w in the place of the loss, z_0 in the place of z_K); rho_0 (the
chain's initial momentum) is held to the same z bars by a second compare_losses call.  Parameter sets have every leaf non-trivial
(hais_restatement.make_params: random mean and md — md is non-zero throughout — per-dimension logdiag, eta 0.6, non-uniform
mgridref_y), at the step sizes of tests/test_gpu_hais.py; many_gmm runs at eps = 0.05.

Target draws come from exact_target_draws.  Every parity case here and the L = 3 wrong-chain case were first run on the CPU with the
restatement in float32 against the restatement in float64, and kept only because that comparison alone stays inside the default bars
of compare_losses: worst over the cases rel_max 7.1e-6 (bar 1e-3), z_max / z_scale 3.7e-7 for z_0 and 6.5e-7 for rho_0 (bar 1e-3).  On the
float64 restatement no row of the many_gmm case has an evaluation within ldvi_cases.BAND (500) of the floor: the guard drops no row
(closest: 9.99e3 above the floor).

Seeds of the bracket test: the forward call runs on seeds 1 .. 4096 (synthetic.parity_seeds), the reverse call on seeds
100001 .. 104096 with the target draws of generator seed 11.  Verified on the CPU with the float64 restatements before they were
fixed here: forward mean(-loss) = -9.5263 (se 0.2449), reverse mean(w) = +2.3384 (se 0.0309) (BRACKET_FORWARD / BRACKET_REVERSE)."""
import ctypes as C
import functools
import math
import re

import numpy as np
import pytest
import torch

import hais_restatement as hr
import reverse_hais_restatement as rh
from cmcd_amd import _lib, hais, reverse_hais, synthetic
from cmcd_amd.model_handler import exact_target_draws, load_model
from helpers import check_stats, compare_losses
from test_reverse_hais_oracle import ORACLE_TARGET

# (dim, eps, q's sigma, scale of q's mean): tests/test_gpu_hais.py's, many_gmm at eps 0.05
TARGETS = {"gmm": (2, 0.05, 2.0, 1.0), "funnel": (10, 0.05, 1.0, 0.5), "many_gmm": (2, 0.05, 15.0, 5.0)}
BRACKET_N = 4096
BRACKET_REVERSE_SEED0 = 100001
BRACKET_DRAW_SEED = 11
# float64 restatements on the bracket's inputs (gmm, K = 8, L = 1; CPU): mean and standard error
BRACKET_FORWARD = (-9.5263, 0.2449)      # mean(-loss) of hais_restatement.forward on seeds 1 .. 4096: 38 standard errors below 0
BRACKET_REVERSE = (+2.3384, 0.0309)      # mean(w) of reverse_chain_hais: 75 standard errors above 0


@functools.lru_cache(maxsize=None)
def target_of(name):
    return load_model(name)[0]


@functools.lru_cache(maxsize=None)
def built(name, K, L, eta=0.6, device="cuda"):
    dim, eps, sigma, mean_scale = TARGETS[name]
    flat, un, fixed = hr.make_params(dim, K, L, eps, seed=K + 10 * L, device=device, mean_scale=mean_scale, sigma=sigma, eta=eta)
    return flat, un, fixed


@functools.lru_cache(maxsize=None)
def target_draws(name, n, seed=5):
    return exact_target_draws(name, load_model(name, None)[2], seed, n, TARGETS[name][0])


def run_device(name, K, L, seeds, x, **kw):
    flat, un, fixed = built(name, K, L, **kw)
    xs = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()
    out = reverse_hais.bound_reverse(torch.from_numpy(np.asarray(seeds, np.int32)).cuda(), xs, flat, un, fixed, target_of(name))
    torch.cuda.synchronize()
    return out


def run_ref(name, K, L, seeds, x, chain=rh.reverse_chain_hais, device="cuda", **kw):
    flat, un, fixed = built(name, K, L, device=device, **kw)
    return rh.run_restatement(flat, un, fixed, ORACLE_TARGET[name](), seeds, x, chain=chain)


def bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def compare(tag, K, w, z0, rho0, ref):
    w_ref, z_ref, rho_ref = ref
    w, z0, rho0 = (t.cpu().numpy() for t in (w, z0, rho0))
    print(tag, "w[:4]", w[:4], "ref", w_ref[:4])
    print(tag, "z0  ", compare_losses(w, w_ref, z0, z_ref, tag, K=K))
    print(tag, "rho0", compare_losses(w, w_ref, rho0, rho_ref, tag + " (rho_0)", K=K))


# --------------------------------------------------------------------------- parity
# (target, n, K, L, eta): n = 300 needs a second workgroup (19 tiles, four per workgroup)
PARITY = [("gmm", n, K, L, 0.6) for n in (1, 16, 37) for K in (1, 8) for L in (1, 3)] + [
    ("funnel", 37, 8, 2, 0.6),
    ("many_gmm", 37, 8, 1, 0.6),
    ("gmm", 300, 2, 1, 0.6),
    ("gmm", 37, 8, 1, 0.0),
]


def parity_inputs(name, n):
    return synthetic.parity_seeds(n) + 40, target_draws(name, n)


@pytest.mark.gpu
@pytest.mark.parametrize("name,n,K,L,eta", PARITY)
def test_parity_with_the_restatement(hip_lib, name, n, K, L, eta):
    tag = f"{name} n={n} K={K} L={L} eta={eta}"
    seeds, x = parity_inputs(name, n)
    w, z0, rho0, st = run_device(name, K, L, seeds, x, eta=eta)
    ref = run_ref(name, K, L, seeds, x, eta=eta)
    compare(tag, K, w, z0, rho0, ref)
    print(tag, check_stats(st, w, tag))
    flat, un, fixed = built(name, K, L, eta=eta)
    eubo, (w2, z2) = reverse_hais.compute_reverse_bound(torch.from_numpy(seeds).cuda(), torch.from_numpy(x).cuda(), flat, un, fixed,
                                                        target_of(name))
    assert abs(float(eubo) - ref[0].mean()) <= 1e-3 * max(1.0, abs(ref[0].mean()))
    assert torch.equal(bits(w2), bits(w)) and torch.equal(bits(z2), bits(z0))


# --------------------------------------------------------------------------- the wrong chain
@pytest.mark.gpu
def test_the_inner_kicks_are_full_kicks(hip_lib):
    """At L = 3 the device matches the right restatement (parity above: gmm n = 37, K = 8, L = 3) and is more than 100 bars away from
    the chain that treats every inner kick as a half-kick (tests/test_reverse_hais_oracle.py measures 0.74 against the bar of 1e-3)."""
    n, K, L = 37, 8, 3
    seeds, x = np.arange(1, n + 1, dtype=np.int32), target_draws("gmm", n)
    w, z0, rho0, _ = run_device("gmm", K, L, seeds, x)
    compare("L = 3", K, w, z0, rho0, run_ref("gmm", K, L, seeds, x))
    w_bad, _, _ = run_ref("gmm", K, L, seeds, x, chain=rh.reverse_chain_hais_inner_half_kicks)
    wd = w.double().cpu().numpy()
    assert (np.abs(w_bad - wd) / np.maximum(1.0, np.abs(wd))).max() > 0.1


# --------------------------------------------------------------------------- non-finite rows
@pytest.mark.gpu
@pytest.mark.parametrize("whole_tile", [False, True])
def test_non_finite_rows_weigh_nothing(hip_lib, whole_tile):
    name, K, L, n = "many_gmm", 8, 1, 49
    seeds = synthetic.parity_seeds(n)
    x = target_draws(name, n)
    clean_w, clean_z, clean_rho, _ = run_device(name, K, L, seeds, x)
    bad = [3, 20] + (list(range(32, 48)) if whole_tile else [])
    x = x.copy()
    x[3, 1] = np.nan
    x[20, 0] = np.inf
    for r in bad[2:]:
        x[r, r % 2] = np.nan if r % 3 else -np.inf
    w, z0, rho0, st = run_device(name, K, L, seeds, x)
    wc, good = w.cpu().numpy(), np.setdiff1d(np.arange(n), bad)
    assert np.all(wc[bad] == np.inf) and not np.isnan(wc).any()
    assert np.isfinite(wc[good]).all()
    for got, ref in ((w, clean_w), (z0, clean_z), (rho0, clean_rho)):
        assert torch.equal(bits(got[good]), bits(ref[good]))
    s = st.cpu().numpy()
    assert not np.isnan(s).any() and s[0] == n - len(bad) and s[1] == np.inf
    check_stats(st, w, "non-finite rows")
    flat, un, fixed = built(name, K, L)
    eubo, _ = reverse_hais.compute_reverse_bound(torch.from_numpy(seeds).cuda(), torch.from_numpy(x).cuda(), flat, un, fixed,
                                                 target_of(name))
    assert float(eubo) == np.inf


# --------------------------------------------------------------------------- determinism and plumbing
@pytest.fixture(scope="module")
def funnel_case():
    name, K, L, n = "funnel", 8, 2, 300
    flat, un, fixed = built(name, K, L)
    seeds = torch.from_numpy(synthetic.parity_seeds(n)).cuda()
    x = torch.from_numpy(target_draws(name, n)).cuda()
    args = (flat, un, fixed, target_of(name))
    out = reverse_hais.bound_reverse(seeds, x, *args)
    torch.cuda.synchronize()
    return seeds, x, args, out


@pytest.mark.gpu
def test_repeated_calls_give_equal_bits(funnel_case):
    seeds, x, args, first = funnel_case
    again = reverse_hais.bound_reverse(seeds, x, *args)
    torch.cuda.synchronize()
    assert len(first) == 4
    for a, c in zip(first, again):
        assert torch.equal(bits(a), bits(c))


@pytest.mark.gpu
def test_a_particle_does_not_depend_on_its_batch(funnel_case):
    seeds, x, args, whole = funnel_case
    rows = torch.arange(100, 117, device="cuda")       # 17 rows that straddle two tiles of the large batch
    w, z0, rho0, _ = reverse_hais.bound_reverse(seeds[rows].contiguous(), x[rows].contiguous(), *args)
    torch.cuda.synchronize()
    for got, ref in zip((w, z0, rho0), whole):
        assert torch.equal(bits(got), bits(ref[rows]))


@pytest.mark.gpu
def test_graph_capture_and_replay(funnel_case):
    seeds, x, args, eager = funnel_case
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        reverse_hais.bound_reverse(seeds, x, *args)      # allocator warm-up on a side stream
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = reverse_hais.bound_reverse(seeds, x, *args)
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
        out = reverse_hais.bound_reverse(seeds, x, *args)
    side.synchronize()
    for a, c in zip(eager, out):
        assert torch.equal(bits(a), bits(c))


# --------------------------------------------------------------------------- the bracket
def bracket_reverse_inputs():
    n = BRACKET_N
    return np.arange(BRACKET_REVERSE_SEED0, BRACKET_REVERSE_SEED0 + n, dtype=np.int32), target_draws("gmm", n, seed=BRACKET_DRAW_SEED)


@functools.lru_cache(maxsize=None)
def bracket_reference():
    """The float64 restatements on the bracket's inputs (gmm, K = 8, L = 1) -> (-loss[N], w[N])."""
    flat, un, fixed = built("gmm", 8, 1, device="cpu")
    loss, _ = hr.forward(synthetic.parity_seeds(BRACKET_N), hr.params_numpy(un, flat), 2, 8, 1, "gmm")
    seeds, x = bracket_reverse_inputs()
    return -loss, run_ref("gmm", 8, 1, seeds, x, device="cpu")[0]


@pytest.mark.gpu
def test_elbo_and_eubo_bracket_ln_z(hip_lib):
    """gmm is normalised (ln Z = 0): E_Q[-loss] < 0 < E_P[w]; on the float64 restatements each mean lies more than 5 of its standard
    errors away from 0 (BRACKET_FORWARD, BRACKET_REVERSE), and the device's means are within 1e-3 max(1, |ref|) of them."""
    n = BRACKET_N
    flat, un, fixed = built("gmm", 8, 1)
    args = (flat, un, fixed, target_of("gmm"))
    loss, _, _ = hais.bound_forward(torch.from_numpy(synthetic.parity_seeds(n)).cuda(), *args)
    seeds, x = bracket_reverse_inputs()
    w, _, _, st = reverse_hais.bound_reverse(torch.from_numpy(seeds).cuda(), torch.from_numpy(x).cuda(), *args)
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
def test_unsupported_configurations_raise(hip_lib):
    n = 32
    seeds = torch.arange(1, n + 1, dtype=torch.int32, device="cuda")
    x = torch.zeros((n, 2), device="cuda")
    flat, un, fixed = built("gmm", 8, 1)
    with pytest.raises(ValueError, match="nbridges"):                       # nbridges = 0: the mean-field bound has no chain
        reverse_hais.bound_reverse(seeds, x, flat, un, (2, 0, 1), target_of("gmm"))
    with pytest.raises(ValueError, match="lfsteps"):
        reverse_hais.bound_reverse(seeds, x, flat, un, (2, 8, 0), target_of("gmm"))
    with pytest.raises(ValueError, match="target dim"):
        reverse_hais.bound_reverse(seeds, x, flat, un, fixed, target_of("funnel"))
    # a (target, dim) without an instance, through the C level (the Python layer cannot build one): gmm at dim 3, and lgcp
    L = _lib.lib()
    assert L.cmcd_reverse_hais_workspace_bytes(0, 3, 8, 1, n) == 0 and "kernel instance" in _lib.last_error()
    assert L.cmcd_reverse_hais_workspace_bytes(3, 1600, 8, 1, n) == 0 and "lgcp" in _lib.last_error()
    from helpers import lgcp_counts_fixture
    from cmcd_amd.lgcp import load_model_lgcp
    tgt, dim = load_model_lgcp("lgcp", None, flat_bin_counts=lgcp_counts_fixture())[:2]
    pf, pu, pfix = hr.make_params(dim, 2, 1, 1e-3, device="cuda")
    with pytest.raises(NotImplementedError, match="lgcp"):
        reverse_hais.bound_reverse(seeds, torch.zeros((n, dim), device="cuda"), pf, pu, pfix, tgt)


@pytest.mark.gpu
def test_bad_inputs_fail_before_any_launch(hip_lib):
    flat, un, fixed = built("gmm", 8, 1)
    n = 32
    seeds = torch.arange(1, n + 1, dtype=torch.int32, device="cuda")
    args = (flat, un, fixed, target_of("gmm"))
    good = torch.zeros((n, 2), device="cuda")
    with pytest.raises(RuntimeError, match="ROCm device"):
        reverse_hais.bound_reverse(seeds, good.cpu(), *args)
    with pytest.raises(ValueError, match="shape"):
        reverse_hais.bound_reverse(seeds, torch.zeros((n, 3), device="cuda"), *args)
    with pytest.raises(ValueError, match="shape"):
        reverse_hais.bound_reverse(seeds, torch.zeros((n + 1, 2), device="cuda"), *args)
    with pytest.raises(ValueError, match="float32"):
        reverse_hais.bound_reverse(seeds, good.double(), *args)
    with pytest.raises(ValueError, match="contiguous"):
        reverse_hais.bound_reverse(seeds, torch.zeros((2, n), device="cuda").t(), *args)
    # the C level: a workspace one byte short, a null x
    L = _lib.lib()
    lay = hais._layout(un)
    need = L.cmcd_reverse_hais_workspace_bytes(0, 2, 8, 1, n)
    assert need == 2 * 5 * 8      # two tiles, one 5-double record each
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    from cmcd_amd import mcdboundingmachine as mcdbm
    w, z0, st = mcdbm._outputs(n, 2, good.device)
    rho0 = torch.empty_like(z0)
    w.fill_(7.0)

    def call(x_ptr, ws_bytes):
        return L.cmcd_bound_reverse_hais(0, 2, 8, 1, lay, seeds.data_ptr(), x_ptr, n, flat.data_ptr(), flat.numel(), None, 0,
                                         ws.data_ptr(), ws_bytes, w.data_ptr(), z0.data_ptr(), rho0.data_ptr(), st.data_ptr(), None)

    assert call(good.data_ptr(), need - 1) == -3 and "workspace too small" in _lib.last_error()
    assert call(None, need) == -1 and "null pointer" in _lib.last_error()
    torch.cuda.synchronize()
    assert bool((w == 7.0).all())                 # nothing ran
    assert call(good.data_ptr(), need) == 0
    torch.cuda.synchronize()
    assert bool((w != 7.0).all())


# --------------------------------------------------------------------------- the driver
DRIVER_ARGV = ["--config.model", "gmm", "--config.boundmode", "UHA", "--config.N", "16", "--config.nbridges", "4", "--config.lfsteps", "2",
               "--config.mfvi_iters", "20", "--config.iters", "20", "--config.n_samples", "32", "--config.n_input_dist_seeds", "3",
               "--config.init_eps", "0.01", "--config.lr", "0.001", "--noconfig.compute_w2"]


@pytest.mark.gpu
def test_driver_prints_the_reverse_chain_line_behind_its_flag(hip_lib, capsys):
    from cmcd_amd import main as cli
    elbo, ln_z = cli.main(cli.parse_flags(DRIVER_ARGV + ["--config.eubo_uha"], cli.get_config()))
    out = capsys.readouterr().out
    assert math.isfinite(elbo) and math.isfinite(ln_z)
    m = re.search(r"Reverse chain: EUBO (\S+), reverse ln Z (\S+), reverse ESS (\S+) \(", out)
    assert m, out
    assert all(math.isfinite(float(v)) for v in m.groups()), m.groups()
    assert out.count("Reverse chain") == 1
