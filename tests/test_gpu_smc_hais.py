"""Resumable segments of UHA, Hamiltonian AIS (include/cmcd_hip.h: cmcd_bound_segment_hais) and their SMC driver
(cmcd_amd/smc_hais.py) on the GPU, against the float64 restatement of tests/smc_hais_restatement.py, which
tests/test_smc_ldvi_hais_oracle.py pins on the CPU.  The reference has no such call.  Mirrors tests/test_gpu_smc_uha.py item for item
(the bodies are tests/smc_momentum_checks.py's, shared with tests/test_gpu_smc_ldvi.py); parity goes through
helpers.compare_losses / check_stats unchanged, with -(wpath + lg) in the place of the loss.  The state's rho is the momentum between
bridges and lg carries no momentum term.

Parameter sets have every leaf non-trivial (hais_restatement.make_params, as tests/test_gpu_reverse_hais.py uses it: random mean and
md, per-dimension logdiag, eta 0.6, non-uniform mgridref_y), at that file's step sizes; many_gmm runs at eps = 0.05.

Case selection (python tests/test_gpu_smc_hais.py prints it, no GPU needed).  Every parity case was first run on the CPU with the
restatement in float32 against the restatement in float64 and kept only because that comparison alone stays inside the default bars
of compare_losses.  Worst over the cases: loss rel_max 6.2e-06 (bar 1e-3), z_max / z_scale 5.0e-07, rho 3.8e-06, wpath 1.6e-05, lg
3.3e-06 (bars 1e-3).  On the float64 restatement no row of the many_gmm case has an evaluation within ldvi_cases.BAND (500) of the
floor.

Against the forward call: on the MI355X the whole-chain segment returned the bits of hais.bound_forward in the losses and in z_K on
all three configurations (the two kernels run the same expressions in the same order); the test does not require it.

Fixed seeds (checked on the CPU by tests/test_smc_ldvi_hais_oracle.py, float64 restatement):
  * FLOOR_*: many_gmm under make_params(sigma = 60, mean_scale = 5, seed = 18), eps 0.05, L = 1, seeds 1 .. 512 in 2 groups, K = 8,
    cuts at every bridge, ess_threshold = 1, resampling seed 5: 24 particles have lg = -inf at the first cut, one ancestor of the
    first stage has 25 offspring, every stage resamples both groups, ln Z = (0.088, 0.151).
  * UNBIASED_*: gmm under make_params(sigma = 2, mean_scale = 1, seed = 18), eps 0.05, L = 1, seeds 100001 .. 116384 in 64 groups of
    256, K = 8, cuts at every bridge, ess_threshold = 0.5: 79 resampling events, mean_g exp(ln Z_g) = 1.0297, std_g = 0.4464, i.e.
    |mean - 1| = 0.53 std / sqrt(64) <= 2 std / sqrt(64)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

if __name__ == "__main__":      # run as a script: the repository root is not on the path yet (under pytest conftest.py puts it there)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import hais_restatement as hr
import ldvi_cases
import smc_hais_restatement as rh
import smc_momentum_checks as chk
from cmcd_amd import hais, smc, smc_hais, smc_ldvi, smc_uha, synthetic
from cmcd_amd.model_handler import load_model
from test_reverse_hais_oracle import ORACLE_TARGET

# (dim, eps, q's sigma, scale of q's mean): tests/test_gpu_reverse_hais.py's
TARGETS = {"gmm": (2, 0.05, 2.0, 1.0), "funnel": (10, 0.05, 1.0, 0.5), "many_gmm": (2, 0.05, 15.0, 5.0)}
FLOOR_SIGMA, FLOOR_SEEDS, FLOOR_CUTS, FLOOR_RESAMPLE_SEED = 60.0, synthetic.parity_seeds(512), list(range(1, 8)), 5
UNBIASED_GROUPS, UNBIASED_M, UNBIASED_RESAMPLE_SEED = 64, 256, 0


def unbiased_seeds():
    return np.arange(100001, 100001 + UNBIASED_GROUPS * UNBIASED_M, dtype=np.int32)


# --------------------------------------------------------------------------- plumbing
@functools.lru_cache(maxsize=None)
def target_of(name):
    return load_model(name)[0]


@functools.lru_cache(maxsize=None)
def built(name, K, L, eta=0.6, device="cuda", sigma=None):
    """-> a record {flat, un, fixed, name}: make_params with the seed rule of tests/test_gpu_reverse_hais.py (K + 10 L)."""
    dim, eps, sig, mean_scale = TARGETS[name]
    flat, un, fixed = hr.make_params(dim, K, L, eps, seed=K + 10 * L, device=device, mean_scale=mean_scale,
                                     sigma=sig if sigma is None else sigma, eta=eta)
    return dict(flat=flat, un=un, fixed=fixed, name=name)


def args_of(b):
    return (b["flat"], b["un"], b["fixed"], target_of(b["name"]))


def runner(b, dtype=np.float64):
    return rh.segment_runner(b["flat"], b["un"], b["fixed"], ORACLE_TARGET[b["name"]](), dtype=dtype)


def forward(b, seeds):
    return hais.bound_forward(seeds, *args_of(b))[:2]


KIT = chk.Kit(smc=smc_hais, args_of=args_of, runner=runner, K_of=lambda b: b["fixed"][1], forward=forward)


# --------------------------------------------------------------------------- 1. parity
# (target, n, K, L, eta, (k0, k1)): the shapes of tests/test_gpu_reverse_hais.py — n = 300 needs a second workgroup (19 tiles, four per
# workgroup) — with the segments (0, K), (0, 1), (K-1, K) and (1, K-1) dealt over them
def _segment_of(i, K):
    return [(0, K), (0, 1), (K - 1, K), (1, K - 1)][i % 4] if K > 2 else [(0, K), (K - 1, K)][i % 2]


PARITY = [("gmm", n, K, L, 0.6) for n in (1, 16, 37) for K in (1, 8) for L in (1, 3)] + [
    ("funnel", 37, 8, 2, 0.6),
    ("many_gmm", 37, 8, 1, 0.6),
    ("gmm", 300, 2, 1, 0.6),
    ("gmm", 37, 8, 1, 0.0),
]
PARITY = [c + (_segment_of(i, c[2]),) for i, c in enumerate(PARITY)]


def _id(c):
    return "%s-n%d-k%d-l%d-eta%g-%d_%d" % (c[:5] + c[5])


@pytest.mark.gpu
@pytest.mark.parametrize("case", PARITY, ids=_id)
def test_parity_with_the_restatement(case):
    name, n, K, L, eta, (k0, k1) = case
    chk.check_parity(KIT, built(name, K, L, eta=eta), _id(case), synthetic.parity_seeds(n) + 40, k0, k1)


# --------------------------------------------------------------------------- 2, 3. composition bits and the key
@pytest.fixture(scope="module", params=["gmm-k8", "funnel-k64", "gmm-k8-l3"])
def whole(request):
    b, n = {"gmm-k8": (("gmm", 8, 1), 33), "funnel-k64": (("funnel", 64, 1), 17), "gmm-k8-l3": (("gmm", 8, 3), 33)}[request.param]
    b = built(*b)
    seeds = synthetic.parity_seeds(n)
    return b, seeds, chk.run_device(KIT, b, chk.dev_seeds(seeds), 0, b["fixed"][1])


@pytest.mark.gpu
def test_two_segments_give_the_bits_of_one(whole):
    b, seeds, full = whole
    chk.check_composition(KIT, b, seeds, full)


# --------------------------------------------------------------------------- 4. the forward call
@pytest.mark.gpu
@pytest.mark.parametrize("name,K,n", [("gmm", 8, 300), ("funnel", 8, 49), ("many_gmm", 8, 512)])
def test_the_whole_segment_matches_the_forward_call(name, K, n):
    chk.check_against_the_forward_call(KIT, built(name, K, 1), n, name)


# --------------------------------------------------------------------------- 5. invariances
@pytest.fixture(scope="module")
def staged():
    """funnel, K = 8, L = 2, 304 particles in 2 groups: the state at bridge 3 and one stage from it (resample, then bridges [3, 6))."""
    return chk.make_staged(KIT, built("funnel", 8, 2))


@pytest.mark.gpu
def test_repeated_calls_give_equal_bits(staged):
    chk.check_repeated_calls(KIT, staged)


@pytest.mark.gpu
def test_a_particle_does_not_depend_on_its_batch(staged):
    chk.check_batch_independence(KIT, staged)


@pytest.mark.gpu
def test_a_stage_moves_rho_with_z_and_leaves_the_input_state_alone(staged):
    chk.check_stage_moves_rho_with_z(KIT, staged)


@pytest.mark.gpu
def test_non_default_stream(staged):
    chk.check_side_stream(KIT, staged)


@pytest.mark.gpu
def test_one_stage_is_captured_and_replayed(staged):
    chk.check_capture(KIT, staged)


# --------------------------------------------------------------------------- 6. the driver, step by step
@pytest.mark.gpu
def test_the_driver_is_segments_and_resampling_stages_as_in_the_restatement():
    chk.check_driver(KIT, built("gmm", 8, 1))


@pytest.mark.gpu
def test_without_resampling_the_driver_is_the_single_segment(whole):
    b, seeds, full = whole
    chk.check_driver_without_resampling(KIT, b, seeds, full)


# --------------------------------------------------------------------------- 7. floor particles
@pytest.mark.gpu
def test_floor_particles_are_resampled_away():
    chk.check_floor(KIT, built("many_gmm", 8, 1, sigma=FLOOR_SIGMA), FLOOR_SEEDS, FLOOR_CUTS, FLOOR_RESAMPLE_SEED)


# --------------------------------------------------------------------------- 8. unbiasedness
@pytest.mark.gpu
def test_exp_ln_z_is_unbiased_on_gmm():
    chk.check_unbiased(KIT, built("gmm", 8, 1), unbiased_seeds(), UNBIASED_GROUPS, UNBIASED_RESAMPLE_SEED)


# --------------------------------------------------------------------------- 9. the NaN rule
@pytest.mark.gpu
def test_a_nan_group_is_left_alone_and_reports_nan():
    chk.check_nan_rule(KIT, built("gmm", 8, 1))


# --------------------------------------------------------------------------- refusals that need the Python layer
@pytest.mark.gpu
def test_unsupported_configurations_raise():
    seeds = chk.dev_seeds(synthetic.parity_seeds(32))
    b = built("gmm", 8, 1)
    flat, un, fixed, tgt = args_of(b)
    mcd_args = lambda bb: (bb["params_flat"], bb["unflatten"], bb["params_fixed"], bb["target"])
    for mode, where in (("MCD_CAIS_sn", r"cmcd_amd\.smc\)"), ("MCD_ULA", r"cmcd_amd\.smc\)"), ("MCD_CAIS_UHA_sn", "cmcd_amd.smc_uha")):
        with pytest.raises(NotImplementedError, match=where):                     # the MCD modes
            smc_hais.segment(seeds, 0, 2, *mcd_args(synthetic.build("gmm_n300_k8", device="cuda", boundmode=mode)))
    bl = synthetic.build("gmm_n300_k8", device="cuda", boundmode="MCD_CAIS_UHA_sn")
    dim, K, _, spec = bl["params_fixed"]
    with pytest.raises(NotImplementedError, match="cmcd_amd.smc_ldvi"):          # LDVI
        smc_hais.segment(seeds, 0, 2, bl["params_flat"], bl["unflatten"], (dim, K, "MCD_U_a-lp-sn", spec), bl["target"])
    from helpers import lgcp_counts_fixture
    lg = synthetic.build("lgcp_n20_k128", device="cuda", lgcp_counts=lgcp_counts_fixture(), boundmode="MCD_CAIS_UHA_sn", nbridges=2)
    fl, ul, fx = hais.initialize(dim=1600, nbridges=2, lfsteps=1, eps=0.01, eta=0.5, device="cuda")
    with pytest.raises(NotImplementedError, match="lgcp"):
        smc_hais.segment(seeds, 0, 2, fl, ul, fx, lg["target"])
    f3, u3, x3 = hais.initialize(dim=10, nbridges=8, lfsteps=1, eps=0.05, eta=0.5, device="cuda")
    with pytest.raises(ValueError, match="target dim"):                           # no widths in this mode: the funnel's q on gmm
        smc_hais.segment(seeds, 0, 2, f3, u3, x3, tgt)
    for k0, k1 in ((0, 9), (3, 3), (-1, 2)):
        with pytest.raises((ValueError, TypeError)):
            smc_hais.segment(seeds if k0 <= 0 else {}, k0, k1, flat, un, fixed, tgt)
    with pytest.raises(ValueError, match="nbridges"):                             # nbridges = 0: the mean-field bound has no chain
        smc_hais.segment(seeds, 0, 1, flat, un, (2, 0, 1), tgt)
    with pytest.raises(ValueError, match="lfsteps"):
        smc_hais.segment(seeds, 0, 2, flat, un, (2, 8, 0), tgt)
    head = chk.run_device(KIT, b, seeds, 0, 2)
    without = {f: head[f] for f in ("z", "wpath", "key")}                          # an overdamped state: no momentum
    with pytest.raises(TypeError, match="rho"):
        smc_hais.segment(without, 2, 4, flat, un, fixed, tgt)
    with pytest.raises(TypeError, match="rho"):
        smc_hais.resample_stage(dict(without, lg=head["lg"]), groups=1)
    with pytest.raises(ValueError, match="cuts"):
        smc_hais.smc_bound(seeds, flat, un, fixed, tgt, cuts=[0, 3])
    for other in (smc, smc_uha, smc_ldvi):                                         # ... and the other three refuse this boundmode
        with pytest.raises((NotImplementedError, ValueError, TypeError)):
            other.segment(seeds, 0, 2, flat, un, fixed, tgt)


# --------------------------------------------------------------------------- the evaluation driver
@pytest.mark.gpu
def test_main_runs_the_smc_evaluation_for_uha(capsys):
    """python -m cmcd_amd.main --config.boundmode UHA --config.smc_eval: the SMC line is printed (it used to be skipped silently for
    this boundmode) and its figures are finite."""
    chk.check_command_line("UHA", capsys, smc_hais, extra=("--config.lfsteps", "2"))


# --------------------------------------------------------------------------- case selection, on the CPU
@functools.lru_cache(maxsize=None)
def float32_gaps():
    """{case id: the restatement in float32 against float64} — raises when a case is outside compare_losses' default bars; the
    many_gmm case must also pass the band guard of tests/ldvi_cases.py on every row."""
    out = {}
    for case in PARITY:
        name, n, K, L, eta, (k0, k1) = case
        b = built(name, K, L, eta=eta, device="cpu")
        seeds = synthetic.parity_seeds(n) + 40
        if name == "many_gmm":
            trace = {}
            runner(b)(seeds, 0, k1, trace=trace)
            assert (np.abs(np.stack(trace["lp"]) - ldvi_cases.FLOOR) > ldvi_cases.BAND).all()
        out[_id(case)] = chk.float32_gap(runner(b, dtype=np.float32), runner(b), seeds, k0, k1)
    return out


if __name__ == "__main__":
    gaps = float32_gaps()
    for tag, g in gaps.items():
        print(tag, {k: "%.1e" % v for k, v in g.items()})
    print("worst", {k: "%.1e" % max(g[k] for g in gaps.values()) for k in next(iter(gaps.values()))})
