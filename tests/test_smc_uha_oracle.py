"""Pins tests/smc_uha_restatement.py (the float64 yardstick of cmcd_bound_segment_uha and cmcd_amd.smc_uha) without a device:
composed over any cut set, `segment_chain` is the forward oracle of the mode (oracle.compute_log_elbo_batch_uha); an intermediate
lg is the geometric bridge plus the momentum's density; the driver with ess_threshold = 0 is the plain chain and its ln Z is
oracle.ln_z; and the seeds tests/test_gpu_smc_uha.py fixes for its floor and unbiasedness cases have the properties it relies on.

Measured on the restatement (float64), for the seed sets of tests/test_gpu_smc_uha.py:
  * FLOOR_*: many_gmm dds, init_sigma = 60, init_eps = 0.05, seeds 1 .. 512 in 2 groups, K = 8, cuts at every bridge,
    ess_threshold = 1, resampling seed 5: 10 particles have lg = -inf at the first cut, one ancestor of the first stage has 27
    offspring, every one of the 7 stages resamples both groups, ln Z = (-0.402, 0.762), no NaN, every final loss finite.
  * UNBIASED_*: gmm with init_sigma = 3, init_eps = 0.1, seeds 100001 .. 116384 in 64 groups of 256, K = 8, cuts at every bridge,
    ess_threshold = 0.5, resampling seed 0: 187 resampling events, mean_g exp(ln Z_g) = 0.9870, std_g = 0.2409, i.e.
    |mean - 1| = 0.43 std / sqrt(64) <= 2 std / sqrt(64)."""
import numpy as np
import pytest

from cmcd_amd import synthetic
from helpers import oracle_target
from oracle import cmcd_oracle as orc
from oracle import prng
import smc_uha_restatement as ru

MODE = "MCD_CAIS_UHA_sn"
# (config, overrides): gmm, funnel and many_gmm; geffner and dds; K of {1, 6, 16}
CASES = [
    ("gmm_n300_k8", dict(nbridges=6)),
    ("gmm_n300_k8", dict(nbridges=1, nn_arch="dds")),
    ("gmm_n300_k8", dict(nbridges=16, emb_dim=40)),
    ("funnel_n300_k64", dict(nbridges=16)),
    ("funnel_n300_k64", dict(nbridges=6, nn_arch="dds")),
    ("funnel_n300_k64", dict(nbridges=1)),
    ("many_gmm_var_n16000_k256", dict(nbridges=6)),
    ("many_gmm_n2000_k256_dds", dict(nbridges=16, init_eps=0.05)),
]


def build(name, **over):
    return synthetic.build(name, device="cpu", dense=True, boundmode=MODE, **over)


def run_oracle(b, seeds):
    dim, K, mode, spec = b["params_fixed"]
    return orc.compute_log_elbo_batch_uha(np.asarray(seeds), synthetic.oracle_params(b["unflatten"], b["params_flat"]), dim, K,
                                          spec.arch, oracle_target(b["cfg"]), dtype=np.float64)


def compose(run, seeds, edges):
    state = run(seeds, 0, edges[0])
    for a, b in zip(edges, edges[1:]):
        state = run(state, a, b)
    return state


def forward_key(seeds, K):
    """gen_K of the 2nd-order forward chain (oracle/prng.py: particle_noise_uha)."""
    _, bb = prng.split(prng.prng_key(seeds))
    c, _ = prng.split(bb)
    _, g1 = prng.split(c)
    _, gen = prng.split(g1)
    for _ in range(K):
        _, h = prng.split(gen)
        _, gen = prng.split(h)
    return gen


@pytest.mark.parametrize("name,over", CASES)
def test_composed_over_any_cut_set_it_is_the_forward_oracle(name, over):
    b = build(name, **over)
    K = b["params_fixed"][1]
    seeds = synthetic.parity_seeds(24)
    loss, zK = run_oracle(b, seeds)
    run = ru.segment_runner(b)
    fin = np.isfinite(loss)
    assert fin.sum() >= 20
    for edges in ([K], [1, K], [K - 1, K], list(range(1, K + 1)), [1, K // 2, K - 1, K]):
        edges = sorted(set(e for e in edges if e >= 1))
        st = compose(run, seeds, edges)
        got = ru.losses_of(st)
        assert np.array_equal(np.isinf(got), np.isinf(loss)), edges
        np.testing.assert_allclose(got[fin], loss[fin], rtol=1e-9, atol=1e-9, err_msg=str(edges))
        np.testing.assert_allclose(st["z"], zK, rtol=1e-9, atol=1e-9, err_msg=str(edges))
        assert np.array_equal(st["key"], forward_key(seeds, K)), edges      # the key a segment hands on is gen_K of the forward chain
        assert st["rho"].shape == st["z"].shape and np.isfinite(st["rho"][fin]).all()


def test_intermediate_lg_is_the_geometric_bridge_plus_the_momentum_density_and_the_floor_gives_minus_inf():
    b = build("many_gmm_n2000_k256_dds", nbridges=4, init_eps=0.05)
    assert b["cfg"]["init_sigma"] == 60.0
    p = synthetic.oracle_params(b["unflatten"], b["params_flat"])
    run = ru.segment_runner(b)
    st = run(synthetic.parity_seeds(200), 0, 2)
    logp, _ = oracle_target(b["cfg"])(st["z"])
    beta = orc.betas_from_grid(p["mgridref_y"], p["gridref_x"], p["target_x"], np.float64)[1]
    floor = logp == -np.inf
    assert floor.any() and not floor.all()            # init_sigma = 60: some particles sit beyond the -1e4 floor
    assert np.all(st["lg"][floor] == -np.inf) and not np.isnan(st["lg"]).any()
    rho = st["rho"][~floor]
    log_n = np.sum(-0.5 * rho * rho - 0.5 * np.log(2.0 * np.pi), -1)
    want = beta * logp[~floor] + (1 - beta) * orc.q_log_prob(p["vd"], st["z"][~floor]) + log_n
    np.testing.assert_allclose(st["lg"][~floor], want, rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize("name,over", [("gmm_n300_k8", {}), ("many_gmm_n2000_k256_dds", dict(nbridges=8, init_eps=0.05))])
def test_driver_without_resampling_is_the_plain_chain(name, over):
    b = build(name, **over)
    K = b["params_fixed"][1]
    groups, m = 3, 32
    seeds = synthetic.parity_seeds(groups * m)
    loss, zK = run_oracle(b, seeds)
    out = ru.smc_chain(seeds, ru.segment_runner(b), K, groups=groups, cuts=[1, K // 2, K - 1], ess_threshold=0.0, seed=3)
    assert not out["resampled"].any() and out["resampled"].shape == (3, groups) and out["ess"].shape == (4, groups)
    assert all(np.array_equal(a, np.arange(groups * m)) for a in out["ancestors"])
    fin = np.isfinite(loss)
    assert np.array_equal(np.isinf(out["losses"]), ~fin)
    np.testing.assert_allclose(out["losses"][fin], loss[fin], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(out["z"], zK, rtol=1e-9, atol=1e-9)
    for g in range(groups):
        assert abs(out["ln_Z"][g] - orc.ln_z(loss[g * m:(g + 1) * m])) <= 1e-9


def test_resampled_groups_restart_with_uniform_weights_move_rho_with_z_and_keep_their_keys():
    b = build("gmm_n300_k8")
    run = ru.segment_runner(b)
    st = run(synthetic.parity_seeds(64), 0, 4)
    new, trig, ess, inc, anc = ru.resample_stage(st, 2, 1.0, 9)
    assert trig.all() and (ess < 32).all()
    assert np.array_equal(new["key"], st["key"])                      # keys stay with their slot
    assert np.array_equal(new["z"], st["z"][anc]) and np.array_equal(new["rho"], st["rho"][anc])
    assert np.all(ru.losses_of(new) == 0.0)
    assert (anc[:32] < 32).all() and (anc[32:] >= 32).all()
    for g in range(2):
        assert abs(inc[g] - orc.ln_z(ru.losses_of(st)[g * 32:(g + 1) * 32])) <= 1e-12


def test_the_seeds_of_the_gpu_floor_case_have_the_properties_it_needs():
    import test_gpu_smc_uha as t
    b = build(t.FLOOR_CONFIG, **t.FLOOR_OVER)
    assert b["cfg"]["init_sigma"] == 60.0 and b["params_fixed"][1] == 8
    out = ru.smc_chain(t.FLOOR_SEEDS, ru.segment_runner(b), 8, groups=2, cuts=t.FLOOR_CUTS, ess_threshold=1.0, seed=t.FLOOR_RESAMPLE_SEED)
    first = out["arrived"][0]
    n_floor = int((first["lg"] == -np.inf).sum())
    most = int(np.bincount(out["ancestors"][0], minlength=512).max())
    print("lg = -inf at the first cut:", n_floor, "most offspring:", most, "events", out["resampled"].sum(0), "ln Z", out["ln_Z"])
    assert n_floor == 10 and most == 27
    assert out["resampled"].all()
    assert not np.isnan(out["losses"]).any() and np.isfinite(out["losses"]).all()


def test_the_seeds_of_the_gpu_unbiasedness_case_pass_with_factor_two():
    import test_gpu_smc_uha as t
    b = build(t.UNBIASED_CONFIG, **t.UNBIASED_OVER)
    K = b["params_fixed"][1]
    out = ru.smc_chain(t.unbiased_seeds(), ru.segment_runner(b), K, groups=t.UNBIASED_GROUPS, cuts=list(range(1, K)),
                       ess_threshold=0.5, seed=t.UNBIASED_RESAMPLE_SEED)
    zhat = np.exp(out["ln_Z"])
    print("mean %.4f std %.4f events %d" % (zhat.mean(), zhat.std(ddof=1), out["resampled"].sum()))
    assert out["resampled"].any()
    assert abs(zhat.mean() - 1.0) <= 2.0 * zhat.std(ddof=1) / np.sqrt(t.UNBIASED_GROUPS), (zhat.mean(), zhat.std(ddof=1))
