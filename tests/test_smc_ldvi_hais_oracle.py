"""Pins tests/smc_ldvi_restatement.py and tests/smc_hais_restatement.py (the float64 yardsticks of cmcd_bound_segment_ldvi /
cmcd_amd.smc_ldvi and cmcd_bound_segment_hais / cmcd_amd.smc_hais) without a device: composed over any cut set, `segment_chain` is
the forward restatement of the mode (tests/ldvi_restatement.py, tests/hais_restatement.py: float64 torch, written from the
reference) in loss and z_K; an intermediate lg is the geometric bridge — plus log N(rho; 0, I) for LDVI, plus nothing for UHA — and
the floor gives -inf; the driver with ess_threshold = 0 is the plain chain; a resampled group restarts with uniform weights, moves
rho with z and keeps its keys; and the seeds tests/test_gpu_smc_ldvi.py and tests/test_gpu_smc_hais.py fix for their floor and
unbiasedness cases have the properties those tests rely on (the measured values are in their docstrings).

The two restatements of a mode differ in how they form the betas: the forward ones place bridge i at (i + 1) / (K + 1) of the grid
in float64, the segment ones read the float32 leaves gridref_x / target_x as the kernels do.  On a grid whose nodes are the bridges
(K <= 32) the two agree to round-off (1e-9 below); at K = 40 on the 33-node grid the float32 abscissae move the betas by 1e-8 and
the losses by 3e-7 (bar 1e-5)."""
import numpy as np
import pytest

import hais_restatement as hr
import ldvi_cases
import ldvi_restatement as lr
import smc_hais_restatement as sh
import smc_ldvi_restatement as sl
from cmcd_amd import synthetic
from helpers import oracle_target
from oracle import cmcd_oracle as orc
from test_reverse_hais_oracle import ORACLE_TARGET
from test_smc_uha_oracle import compose, forward_key

# LDVI: cases of tests/ldvi_cases.py — gmm on 2 and 4 tiles, K of {1, 8, 40}; the funnel; many_gmm; the network-free sibling
LDVI_CASES = ["gmm-n17", "gmm-k1", "gmm-k40", "gmm-w64", "funnel", "many-n33", "nonet", "funnel-nonet"]
# UHA: (target, K, L) with L of {1, 3}; tests/test_gpu_reverse_hais.py's step sizes
HAIS_TARGETS = {"gmm": (2, 0.05, 2.0, 1.0), "funnel": (10, 0.05, 1.0, 0.5), "many_gmm": (2, 0.05, 15.0, 5.0)}
HAIS_CASES = [("gmm", 8, 1), ("gmm", 6, 3), ("gmm", 1, 3), ("funnel", 4, 1), ("funnel", 6, 3), ("many_gmm", 8, 1), ("many_gmm", 4, 3)]


def cut_sets(K):
    return [sorted(set(e for e in edges if e >= 1)) for edges in
            ([K], [1, K], [K - 1, K], list(range(1, K + 1)), [1, K // 2, K - 1, K])]


def hais_built(name, K, L, sigma=None, seed=None):
    dim, eps, sig, mean_scale = HAIS_TARGETS[name]
    return hr.make_params(dim, K, L, eps, seed=K + 10 * L if seed is None else seed, mean_scale=mean_scale,
                          sigma=sig if sigma is None else sigma)


def hais_runner(name, built):
    return sh.segment_runner(*built, ORACLE_TARGET[name]())


# --------------------------------------------------------------------------- composition = the forward restatement
@pytest.mark.parametrize("case_id", LDVI_CASES)
def test_ldvi_composed_over_any_cut_set_it_is_the_forward_restatement(case_id):
    b = ldvi_cases.build(case_id)
    dim, K, mode, _ = b["params_fixed"]
    seeds = synthetic.parity_seeds(24)
    loss, zK = lr.forward(seeds, lr.params_numpy(b["unflatten"], b["params_flat"]), dim, K, b["cfg"]["model"], use_sn=mode == sl.MODES[0])
    run = sl.segment_runner(b)
    fin = np.isfinite(loss)
    assert fin.sum() >= 20
    tol = 1e-9 if K <= 32 else 1e-5
    for edges in cut_sets(K):
        st = compose(run, seeds, edges)
        got = sl.losses_of(st)
        assert np.array_equal(np.isinf(got), np.isinf(loss)), edges
        np.testing.assert_allclose(got[fin], loss[fin], rtol=tol, atol=tol, err_msg=str(edges))
        np.testing.assert_allclose(st["z"][fin], zK[fin], rtol=tol, atol=tol, err_msg=str(edges))
        assert np.array_equal(st["key"], forward_key(seeds, K)), edges      # the key a segment hands on is gen_K of the forward chain
        assert st["rho"].shape == st["z"].shape and np.isfinite(st["rho"][fin]).all()


@pytest.mark.parametrize("name,K,L", HAIS_CASES)
def test_uha_composed_over_any_cut_set_it_is_the_forward_restatement(name, K, L):
    built = hais_built(name, K, L)
    flat, un, (dim, _, _) = built
    seeds = synthetic.parity_seeds(24)
    loss, zK = hr.forward(seeds, hr.params_numpy(un, flat), dim, K, L, name)
    run = hais_runner(name, built)
    fin = np.isfinite(loss)
    assert fin.sum() >= 20
    for edges in cut_sets(K):
        st = compose(run, seeds, edges)
        got = sh.losses_of(st)
        assert np.array_equal(np.isinf(got), np.isinf(loss)), edges
        np.testing.assert_allclose(got[fin], loss[fin], rtol=1e-9, atol=1e-9, err_msg=str(edges))
        np.testing.assert_allclose(st["z"][fin], zK[fin], rtol=1e-9, atol=1e-9, err_msg=str(edges))
        assert np.array_equal(st["key"], forward_key(seeds, K)), edges
        assert st["rho"].shape == st["z"].shape and np.isfinite(st["rho"][fin]).all()


# --------------------------------------------------------------------------- the intermediate lg
def test_ldvi_intermediate_lg_is_the_geometric_bridge_plus_the_momentum_density_and_the_floor_gives_minus_inf():
    import test_gpu_smc_ldvi as t
    b = t.build(t.FLOOR_CONFIG, device="cpu", **dict(t.FLOOR_OVER, nbridges=4))
    assert b["cfg"]["init_sigma"] == 60.0
    p = sl.params_numpy(b["unflatten"], b["params_flat"])
    st = sl.segment_runner(b)(synthetic.parity_seeds(200), 0, 2)
    logp, _ = oracle_target(b["cfg"])(st["z"])
    beta = orc.betas_from_grid(p["mgridref_y"], p["gridref_x"], p["target_x"], np.float64)[1]
    floor = logp == -np.inf
    assert floor.any() and not floor.all()            # init_sigma = 60: some particles sit beyond the -1e4 floor
    assert np.all(st["lg"][floor] == -np.inf) and not np.isnan(st["lg"]).any()
    rho = st["rho"][~floor]
    log_n = np.sum(-0.5 * rho * rho - 0.5 * np.log(2.0 * np.pi), -1)
    want = beta * logp[~floor] + (1 - beta) * orc.q_log_prob(p["vd"], st["z"][~floor]) + log_n
    np.testing.assert_allclose(st["lg"][~floor], want, rtol=1e-13, atol=1e-13)


def test_uha_intermediate_lg_is_the_geometric_bridge_alone_and_the_floor_gives_minus_inf():
    built = hais_built("many_gmm", 4, 1, sigma=60.0)
    flat, un, _ = built
    p = hr.params_numpy(un, flat)
    tgt = ORACLE_TARGET["many_gmm"]()
    st = hais_runner("many_gmm", built)(synthetic.parity_seeds(200), 0, 2)
    logp, _ = tgt(st["z"])
    beta = orc.betas_from_grid(p["mgridref_y"], p["gridref_x"], p["target_x"], np.float64)[1]
    floor = logp == -np.inf
    assert floor.any() and not floor.all()
    assert np.all(st["lg"][floor] == -np.inf) and not np.isnan(st["lg"]).any()
    want = beta * logp[~floor] + (1 - beta) * orc.q_log_prob(p["vd"], st["z"][~floor])      # no momentum term
    np.testing.assert_allclose(st["lg"][~floor], want, rtol=1e-13, atol=1e-13)
    assert np.abs(st["rho"]).max() > 0.1                                                     # ... though the state has a momentum


# --------------------------------------------------------------------------- the driver
def _plain_chain(run, losses_of, loss, zK, K, tol=1e-9):
    groups, m = 3, 32
    out = sl.smc_chain(synthetic.parity_seeds(groups * m), run, K, groups=groups, cuts=[1, K // 2, K - 1], ess_threshold=0.0, seed=3)
    assert not out["resampled"].any() and out["resampled"].shape == (3, groups) and out["ess"].shape == (4, groups)
    assert all(np.array_equal(a, np.arange(groups * m)) for a in out["ancestors"])
    fin = np.isfinite(loss)
    assert np.array_equal(np.isinf(out["losses"]), ~fin)
    np.testing.assert_allclose(out["losses"][fin], loss[fin], rtol=tol, atol=tol)
    np.testing.assert_allclose(out["z"][fin], zK[fin], rtol=tol, atol=tol)
    for g in range(groups):
        assert abs(out["ln_Z"][g] - orc.ln_z(loss[g * m:(g + 1) * m])) <= tol


@pytest.mark.parametrize("case_id", ["gmm-n33", "many-n33"])
def test_ldvi_driver_without_resampling_is_the_plain_chain(case_id):
    b = ldvi_cases.build(case_id)
    dim, K, mode, _ = b["params_fixed"]
    loss, zK = lr.forward(synthetic.parity_seeds(96), lr.params_numpy(b["unflatten"], b["params_flat"]), dim, K, b["cfg"]["model"])
    _plain_chain(sl.segment_runner(b), sl.losses_of, loss, zK, K)


@pytest.mark.parametrize("name,L", [("gmm", 1), ("many_gmm", 3)])
def test_uha_driver_without_resampling_is_the_plain_chain(name, L):
    built = hais_built(name, 8, L)
    flat, un, (dim, K, _) = built
    loss, zK = hr.forward(synthetic.parity_seeds(96), hr.params_numpy(un, flat), dim, K, L, name)
    _plain_chain(hais_runner(name, built), sh.losses_of, loss, zK, K)


@pytest.mark.parametrize("which", ["ldvi", "uha"])
def test_resampled_groups_restart_with_uniform_weights_move_rho_with_z_and_keep_their_keys(which):
    mod, run = (sl, sl.segment_runner(ldvi_cases.build("gmm-n33"))) if which == "ldvi" else (sh, hais_runner("gmm", hais_built("gmm", 8, 1)))
    st = run(synthetic.parity_seeds(64), 0, 4)
    new, trig, ess, inc, anc = mod.resample_stage(st, 2, 1.0, 9)
    assert trig.all() and (ess < 32).all()
    assert np.array_equal(new["key"], st["key"])                      # keys stay with their slot
    assert np.array_equal(new["z"], st["z"][anc]) and np.array_equal(new["rho"], st["rho"][anc])
    assert not np.array_equal(anc, np.arange(64)) and np.all(mod.losses_of(new) == 0.0)
    assert (anc[:32] < 32).all() and (anc[32:] >= 32).all()
    for g in range(2):
        assert abs(inc[g] - orc.ln_z(mod.losses_of(st)[g * 32:(g + 1) * 32])) <= 1e-12


# --------------------------------------------------------------------------- the fixed seeds of the GPU tests
def _floor_properties(out, n, want_floor, want_most):
    first = out["arrived"][0]
    n_floor = int((first["lg"] == -np.inf).sum())
    most = int(np.bincount(out["ancestors"][0], minlength=n).max())
    print("lg = -inf at the first cut:", n_floor, "most offspring:", most, "events", out["resampled"].sum(0), "ln Z", out["ln_Z"])
    assert n_floor >= 1 and most >= 2                 # what the GPU test needs ...
    assert (n_floor, most) == (want_floor, want_most)  # ... and what its docstring records
    assert out["resampled"].all()
    assert not np.isnan(out["losses"]).any() and np.isfinite(out["losses"]).all()


def test_the_seeds_of_the_gpu_floor_cases_have_the_properties_they_need():
    import test_gpu_smc_hais as th
    import test_gpu_smc_ldvi as tl
    b = tl.build(tl.FLOOR_CONFIG, device="cpu", **tl.FLOOR_OVER)
    assert b["cfg"]["init_sigma"] == 60.0 and b["params_fixed"][1] == 8
    out = sl.smc_chain(tl.FLOOR_SEEDS, sl.segment_runner(b), 8, groups=2, cuts=tl.FLOOR_CUTS, ess_threshold=1.0,
                       seed=tl.FLOOR_RESAMPLE_SEED)
    _floor_properties(out, 512, 10, 16)
    bh = th.built("many_gmm", 8, 1, sigma=th.FLOOR_SIGMA, device="cpu")
    out = sh.smc_chain(th.FLOOR_SEEDS, th.runner(bh), 8, groups=2, cuts=th.FLOOR_CUTS, ess_threshold=1.0, seed=th.FLOOR_RESAMPLE_SEED)
    _floor_properties(out, 512, 24, 25)


def _unbiased_with_factor_two(out, groups):
    zhat = np.exp(out["ln_Z"])
    print("mean %.4f std %.4f events %d" % (zhat.mean(), zhat.std(ddof=1), out["resampled"].sum()))
    assert out["resampled"].any()
    assert abs(zhat.mean() - 1.0) <= 2.0 * zhat.std(ddof=1) / np.sqrt(groups), (zhat.mean(), zhat.std(ddof=1))


def test_the_seeds_of_the_gpu_unbiasedness_cases_pass_with_factor_two():
    import test_gpu_smc_hais as th
    import test_gpu_smc_ldvi as tl
    b = tl.build(tl.UNBIASED_CONFIG, device="cpu", **tl.UNBIASED_OVER)
    K = b["params_fixed"][1]
    out = sl.smc_chain(tl.unbiased_seeds(), sl.segment_runner(b), K, groups=tl.UNBIASED_GROUPS, cuts=list(range(1, K)),
                       ess_threshold=0.5, seed=tl.UNBIASED_RESAMPLE_SEED)
    _unbiased_with_factor_two(out, tl.UNBIASED_GROUPS)
    bh = th.built("gmm", 8, 1, device="cpu")
    out = sh.smc_chain(th.unbiased_seeds(), th.runner(bh), 8, groups=th.UNBIASED_GROUPS, cuts=list(range(1, 8)), ess_threshold=0.5,
                       seed=th.UNBIASED_RESAMPLE_SEED)
    _unbiased_with_factor_two(out, th.UNBIASED_GROUPS)


def test_the_gpu_parity_cases_are_inside_the_bars_in_float32_alone():
    """The selection rule of the GPU parity cases: the restatement in float32 against the restatement in float64 stays inside the
    default bars of helpers.compare_losses (float32_gap raises otherwise), with a tenfold margin on wpath, lg and rho."""
    import test_gpu_smc_hais as th
    import test_gpu_smc_ldvi as tl
    for mod in (tl, th):
        for tag, g in mod.float32_gaps().items():
            assert max(g["wpath"], g["lg"], g["rho"], g["z"], g["rel_max"]) <= 1e-4, (tag, g)
