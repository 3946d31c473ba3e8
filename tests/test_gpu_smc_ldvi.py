"""Resumable segments of LDVI (include/cmcd_hip.h: cmcd_bound_segment_ldvi) and their SMC driver (cmcd_amd/smc_ldvi.py) on the GPU,
against the float64 restatement of tests/smc_ldvi_restatement.py, which tests/test_smc_ldvi_hais_oracle.py pins on the CPU.  The
reference has no such call.  Mirrors tests/test_gpu_smc_uha.py item for item (the bodies are tests/smc_momentum_checks.py's, shared
with tests/test_gpu_smc_hais.py); parity goes through helpers.compare_losses / check_stats unchanged, with -(wpath + lg) in the
place of the loss.

Parameter conventions are tests/ldvi_cases.py's: the dense tree; the funnel at eps 0.05, gamma 4; many_gmm on the geffner net at
eps 0.05, gamma 2 and the configuration's own sigma (60), its seeds chosen from 41 .. 104 by the band guard (no evaluation of the
float64 restatement within ldvi_cases.BAND = 500 of the floor of log p: float32 cannot take such a particle across it).

Case selection (python tests/test_gpu_smc_ldvi.py prints it, no GPU needed).  Every parity case was first run on the CPU with the
restatement in float32 against the restatement in float64 and kept only because that comparison alone stays inside the default bars
of compare_losses.  Worst over the cases: loss rel_max 5.7e-06 (bar 1e-3; the K = 40 case, 38 bridges: 2.4e-06, bar 0.2), z_max / z_scale
2.0e-07, rho 4.2e-07, wpath 9.5e-06, lg 1.5e-06 (bars 1e-3).  One candidate was dropped by that rule's margin: many_gmm on 2 tiles with
n = 33 over (1, 7) — one of the seeds 58 .. 73 starts so far out that wpath is the small difference of two large kernel densities, and
float32 alone costs 6.0e-04 of wpath's 1e-3 (the loss itself: 1.8e-06); the case runs with n = 17 (5.9e-07).

Against the forward call: on the MI355X the whole-chain segment does NOT return the bits of ldvi.bound_forward, in the losses or in
z_K, on any of the three configurations (the rotated loop forms the half-kick before the network evaluation and adds
lg = log p + log N(rho) to wpath in one step; the compiler contracts the two kernels' expressions differently); the worst particle
is 6.7e-06 of its loss and 2.4e-07 in z away (bars 1e-3), and the test does not require equal bits.

Fixed seeds (checked on the CPU by tests/test_smc_ldvi_hais_oracle.py, float64 restatement):
  * FLOOR_*: many_gmm, geffner emb 20, init_sigma = 60, eps 0.05, gamma 2, seeds 1 .. 512 in 2 groups, K = 8, cuts at every bridge,
    ess_threshold = 1, resampling seed 5: 10 particles have lg = -inf at the first cut, one ancestor of the first stage has 16
    offspring, every stage resamples both groups, ln Z = (-0.166, 0.548).
  * UNBIASED_*: gmm with init_sigma = 3, init_eps = 0.1, seeds 100001 .. 116384 in 64 groups of 256, K = 8, cuts at every bridge,
    ess_threshold = 0.5: 369 resampling events, mean_g exp(ln Z_g) = 1.0343, std_g = 0.4441, i.e. |mean - 1| = 0.62 std / sqrt(64)
    <= 2 std / sqrt(64)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

if __name__ == "__main__":      # run as a script: the repository root is not on the path yet (under pytest conftest.py puts it there)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import ldvi_cases
import smc_ldvi_restatement as rl
import smc_momentum_checks as chk
from cmcd_amd import ldvi, smc, smc_hais, smc_ldvi, smc_uha, synthetic

SN, PLAIN = "MCD_U_a-lp-sn", "MCD_U_a-lp"
_FUNNEL = dict(init_eps=0.05, init_gamma=4.0)
_MANY = dict(nn_arch="geffner", emb_dim=20, init_eps=0.05, init_gamma=2.0)
FLOOR_CONFIG, FLOOR_OVER = "many_gmm_n2000_k256_dds", dict(_MANY, nbridges=8)
FLOOR_SEEDS = synthetic.parity_seeds(512)
FLOOR_CUTS = list(range(1, 8))
FLOOR_RESAMPLE_SEED = 5
UNBIASED_CONFIG, UNBIASED_OVER = "gmm_n300_k8", dict(init_sigma=3.0, init_eps=0.1)
UNBIASED_GROUPS, UNBIASED_M, UNBIASED_RESAMPLE_SEED = 64, 256, 0
MANY_SCAN = 64      # the many_gmm cases take their seeds from 41 .. 40 + MANY_SCAN by the band guard


def unbiased_seeds():
    return np.arange(100001, 100001 + UNBIASED_GROUPS * UNBIASED_M, dtype=np.int32)


# --------------------------------------------------------------------------- plumbing
def build(name, mode=SN, device="cuda", dense=True, **over):
    b = synthetic.build(name, device=device, dense=dense, boundmode="MCD_CAIS_UHA_sn" if mode == SN else "MCD_ULA", **over)
    dim, K, _, spec = b["params_fixed"]
    b["params_fixed"] = (dim, K, mode, spec)
    return b


def args_of(b):
    return (b["params_flat"], b["unflatten"], b["params_fixed"], b["target"])


def forward(b, seeds):
    return ldvi.bound_forward(seeds, *args_of(b))[:2]


KIT = chk.Kit(smc=smc_ldvi, args_of=args_of, runner=rl.segment_runner, K_of=lambda b: b["params_fixed"][1], forward=forward)


def case_seeds(b, n, k1):
    """parity seeds 41 .. 40 + n; many_gmm: the first n of 41 .. 40 + MANY_SCAN that pass the band guard on the float64 restatement's
    chain [0, k1)."""
    if b["cfg"]["model"] != "many_gmm":
        return synthetic.parity_seeds(n) + 40
    cand = synthetic.parity_seeds(MANY_SCAN) + 40
    trace = {}
    rl.segment_runner(b)(cand, 0, k1, trace=trace)
    keep = (np.abs(np.stack(trace["lp"]) - ldvi_cases.FLOOR) > ldvi_cases.BAND).all(0)
    assert keep.sum() >= n, (keep.sum(), n)
    return cand[keep][:n]


# --------------------------------------------------------------------------- 1. parity
# (id, config, mode, overrides, n, dense, (k0, k1)): n of {1, 15, 16, 17, 33}; K of {1, 2, 8} and one K = 40 on the 33-node grid (the
# interpolation of beta matters there: beta_{k-1} enters lg); the segments (0, K), (0, 1), (K-1, K), (1, K-1); all eight instances:
# gmm on 2 tiles (24 wide) and 4 (emb 29: one unit in the third tile; emb 60: exact fit), many_gmm on 2 and 4, the funnel on 5 (emb
# 45: one unit in the last tile; emb 60: exact fit; emb 48), the three network-free ones.
PARITY = [
    ("gmm-w24-k8-n33-whole", "gmm_n300_k8", SN, {}, 33, True, (0, 8)),
    ("gmm-w24-k8-n17-middle", "gmm_n300_k8", SN, {}, 17, True, (1, 7)),
    ("gmm-w24-k1-n1", "gmm_n300_k8", SN, dict(nbridges=1), 1, False, (0, 1)),
    ("gmm-w33-k8-n15-last", "gmm_n300_k8", SN, dict(emb_dim=29), 15, True, (7, 8)),
    ("gmm-w64-k2-n16-last", "gmm_n300_k8", SN, dict(emb_dim=60, nbridges=2), 16, True, (1, 2)),
    ("gmm-w64-k8-n17-first", "gmm_n300_k8", SN, dict(emb_dim=60), 17, True, (0, 1)),
    ("gmm-w24-k40-n17-middle", "gmm_n300_k8", SN, dict(nbridges=40, init_eps=0.02), 17, True, (1, 39)),
    ("many_gmm-w24-k8-n17-middle", "many_gmm_n2000_k256_dds", SN, dict(_MANY, nbridges=8), 17, True, (1, 7)),
    ("many_gmm-w64-k8-n17-whole", "many_gmm_n2000_k256_dds", SN, dict(_MANY, emb_dim=60, nbridges=8), 17, True, (0, 8)),
    ("funnel-w65-k8-n17-whole", "funnel_n300_k64", SN, dict(_FUNNEL, emb_dim=45, nbridges=8), 17, True, (0, 8)),
    ("funnel-w80-k8-n33-middle", "funnel_n300_k64", SN, dict(_FUNNEL, emb_dim=60, nbridges=8), 33, True, (1, 7)),
    ("funnel-w68-k2-n16-last", "funnel_n300_k64", SN, dict(_FUNNEL, nbridges=2), 16, True, (1, 2)),
    ("nonet-gmm-k8-n33-middle", "gmm_n300_k8", PLAIN, {}, 33, True, (1, 7)),
    ("nonet-funnel-k8-n17-whole", "funnel_n300_k64", PLAIN, dict(_FUNNEL, nbridges=8), 17, True, (0, 8)),
    ("nonet-many_gmm-k8-n15-last", "many_gmm_n2000_k256_dds", PLAIN, dict(_MANY, nbridges=8), 15, True, (7, 8)),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", PARITY, ids=[c[0] for c in PARITY])
def test_parity_with_the_restatement(case):
    tag, name, mode, over, n, dense, (k0, k1) = case
    b = build(name, mode, dense=dense, **over)
    chk.check_parity(KIT, b, tag, case_seeds(b, n, k1), k0, k1)


# --------------------------------------------------------------------------- 2, 3. composition bits and the key
@pytest.fixture(scope="module", params=["gmm-k8", "funnel-k64"])
def whole(request):
    if request.param == "gmm-k8":
        b, n = build("gmm_n300_k8"), 33
    else:
        b, n = build("funnel_n300_k64", init_eps=0.01, init_gamma=4.0), 17
    seeds = synthetic.parity_seeds(n)
    return b, seeds, chk.run_device(KIT, b, chk.dev_seeds(seeds), 0, b["params_fixed"][1])


@pytest.mark.gpu
def test_two_segments_give_the_bits_of_one(whole):
    b, seeds, full = whole
    chk.check_composition(KIT, b, seeds, full)


# --------------------------------------------------------------------------- 4. the forward call
@pytest.mark.gpu
@pytest.mark.parametrize("name,over,n", [("gmm_n300_k8", {}, 300), ("funnel_n300_k64", dict(_FUNNEL, nbridges=8), 49),
                                          ("many_gmm_n2000_k256_dds", dict(_MANY, nbridges=8), 512)])
def test_the_whole_segment_matches_the_forward_call(name, over, n):
    chk.check_against_the_forward_call(KIT, build(name, **over), n, name)


# --------------------------------------------------------------------------- 5. invariances
@pytest.fixture(scope="module")
def staged():
    """funnel, K = 8, 304 particles in 2 groups: the state at bridge 3 and one stage from it (resample, then bridges [3, 6))."""
    return chk.make_staged(KIT, build("funnel_n300_k64", **dict(_FUNNEL, nbridges=8)))


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
    chk.check_driver(KIT, build("gmm_n300_k8"))


@pytest.mark.gpu
def test_without_resampling_the_driver_is_the_single_segment(whole):
    b, seeds, full = whole
    chk.check_driver_without_resampling(KIT, b, seeds, full)


# --------------------------------------------------------------------------- 7. floor particles
@pytest.mark.gpu
def test_floor_particles_are_resampled_away():
    b = build(FLOOR_CONFIG, **FLOOR_OVER)
    assert b["cfg"]["init_sigma"] == 60.0
    chk.check_floor(KIT, b, FLOOR_SEEDS, FLOOR_CUTS, FLOOR_RESAMPLE_SEED)


# --------------------------------------------------------------------------- 8. unbiasedness
@pytest.mark.gpu
def test_exp_ln_z_is_unbiased_on_gmm():
    chk.check_unbiased(KIT, build(UNBIASED_CONFIG, **UNBIASED_OVER), unbiased_seeds(), UNBIASED_GROUPS, UNBIASED_RESAMPLE_SEED)


# --------------------------------------------------------------------------- 9. the NaN rule
@pytest.mark.gpu
def test_a_nan_group_is_left_alone_and_reports_nan():
    chk.check_nan_rule(KIT, build("gmm_n300_k8"))


# --------------------------------------------------------------------------- refusals that need the Python layer
@pytest.mark.gpu
def test_unsupported_configurations_raise():
    seeds = chk.dev_seeds(synthetic.parity_seeds(32))
    call = lambda b, k0=0, k1=2, state=None: smc_ldvi.segment(seeds if state is None else state, k0, k1, *args_of(b))
    for mode in ("MCD_CAIS_sn", "MCD_CAIS_var_sn", "MCD_ULA", "MCD_ULA_sn"):      # the overdamped modes: cmcd_amd.smc's
        with pytest.raises(NotImplementedError, match=r"cmcd_amd\.smc\)"):
            call(synthetic.build("gmm_n300_k8", device="cuda", boundmode=mode))
    with pytest.raises(NotImplementedError, match="cmcd_amd.smc_uha"):           # 2nd-order CMCD
        call(synthetic.build("gmm_n300_k8", device="cuda", boundmode="MCD_CAIS_UHA_sn"))
    import hais_restatement as hr
    flat, un, fixed = hr.make_params(2, 8, 1, 0.05, device="cuda")
    with pytest.raises(NotImplementedError, match="cmcd_amd.smc_hais"):          # the UHA boundmode
        smc_ldvi.segment(seeds, 0, 2, flat, un, fixed, build("gmm_n300_k8")["target"])
    from helpers import lgcp_counts_fixture
    b = synthetic.build("lgcp_n20_k128", device="cuda", lgcp_counts=lgcp_counts_fixture(), boundmode="MCD_CAIS_UHA_sn", nbridges=2)
    dim, K, _, spec = b["params_fixed"]
    b["params_fixed"] = (dim, K, SN, spec)
    with pytest.raises(NotImplementedError, match="lgcp"):
        call(b)
    with pytest.raises(NotImplementedError, match="geffner"):                     # the dds network
        call(build("gmm_n300_k8", dense=False, nn_arch="dds"))
    with pytest.raises(NotImplementedError):                                      # width 2 * 2 + 130 = 134: 9 tiles, no instance
        call(build("gmm_n300_k8", dense=False, emb_dim=130))
    b = build("gmm_n300_k8", dense=False)
    for k0, k1 in ((0, 9), (3, 3), (-1, 2)):
        with pytest.raises((ValueError, TypeError)):
            call(b, k0, k1, state=seeds if k0 <= 0 else {})
    head = chk.run_device(KIT, b, seeds, 0, 2)
    without = {f: head[f] for f in ("z", "wpath", "key")}                          # an overdamped state: no momentum
    with pytest.raises(TypeError, match="rho"):
        call(b, 2, 4, state=without)
    with pytest.raises(TypeError, match="rho"):
        smc_ldvi.resample_stage(dict(without, lg=head["lg"]), groups=1)
    with pytest.raises(ValueError, match="cuts"):
        smc_ldvi.smc_bound(seeds, *args_of(b), cuts=[0, 3])
    for other in (smc, smc_uha, smc_hais):                                         # ... and the other three refuse this mode
        with pytest.raises((NotImplementedError, ValueError)):
            other.segment(seeds, 0, 2, *args_of(b))


# --------------------------------------------------------------------------- the evaluation driver
@pytest.mark.gpu
def test_main_runs_the_smc_evaluation_for_ldvi(capsys):
    """python -m cmcd_amd.main --config.boundmode MCD_U_a-lp-sn --config.smc_eval: the SMC line is printed (it used to be skipped
    silently for this mode) and its figures are finite."""
    chk.check_command_line(SN, capsys, smc_ldvi)


# --------------------------------------------------------------------------- case selection, on the CPU
@functools.lru_cache(maxsize=None)
def float32_gaps():
    """{case id: the restatement in float32 against float64} — raises when a case is outside compare_losses' default bars."""
    out = {}
    for tag, name, mode, over, n, dense, (k0, k1) in PARITY:
        b = build(name, mode, device="cpu", dense=dense, **over)
        out[tag] = chk.float32_gap(rl.segment_runner(b, dtype=np.float32), rl.segment_runner(b), case_seeds(b, n, k1), k0, k1)
    return out


if __name__ == "__main__":
    gaps = float32_gaps()
    for tag, g in gaps.items():
        print(tag, {k: "%.1e" % v for k, v in g.items()})
    print("worst", {k: "%.1e" % max(g[k] for g in gaps.values()) for k in next(iter(gaps.values()))})
