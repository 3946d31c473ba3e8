"""Pins tests/smc_restatement.py (the float64 yardstick of cmcd_bound_segment and cmcd_amd.smc) without a device: composed over
any cut set, `segment_chain` is the forward oracle; the driver with ess_threshold = 0 is the plain chain and its ln Z is
oracle.ln_z; and the seeds tests/test_gpu_smc.py fixes for its floor and unbiasedness cases have the properties it relies on."""
import numpy as np
import pytest

from cmcd_amd import synthetic
from helpers import oracle_target
from oracle import cmcd_oracle as orc
from oracle import prng
import smc_restatement as rs

# (config, overrides): every overdamped mode, both nets, the three targets, the eps schedules, clipping on and off
CASES = [
    ("gmm_n300_k8", {}),
    ("gmm_n300_k8", dict(boundmode="MCD_ULA_sn")),
    ("gmm_n300_k8", dict(boundmode="MCD_ULA")),
    ("gmm_n300_k8", dict(boundmode="MCD_CAIS_var_sn", nn_arch="dds", eps_schedule="linear", grad_clipping=True)),
    ("funnel_n300_k64", dict(nbridges=16)),
    ("funnel_n300_k64", dict(nbridges=8, nn_arch="dds", boundmode="MCD_ULA_sn")),
    ("many_gmm_var_n16000_k256", dict(nbridges=6)),
    ("many_gmm_n2000_k256_dds", dict(nbridges=12)),
]


def run_oracle(b, seeds):
    """oracle.cmcd_oracle.compute_log_elbo_batch on a synthetic.build() dict, float64, two evaluations per step like the reference"""
    dim, K, mode, spec = b["params_fixed"]
    return orc.compute_log_elbo_batch(np.asarray(seeds), rs.oracle_params(b), dim, K, mode, spec.arch if spec is not None else "dds",
                                      oracle_target(b["cfg"]), eps_schedule=b["cfg"]["eps_schedule"],
                                      grad_clipping=b["cfg"]["grad_clipping"], dtype=np.float64, reuse=False)


def compose(run, seeds, edges):
    state = run(seeds, 0, edges[0])
    for a, b in zip(edges, edges[1:]):
        state = run(state, a, b)
    return state


@pytest.mark.parametrize("name,over", CASES)
def test_composed_over_any_cut_set_it_is_the_forward_oracle(name, over):
    b = synthetic.build(name, device="cpu", dense=True, **over)
    K = b["params_fixed"][1]
    seeds = synthetic.parity_seeds(24)
    loss, zK = run_oracle(b, seeds)
    run = rs.segment_runner(b)
    fin = np.isfinite(loss)
    assert fin.sum() >= 20
    for edges in ([K], [1, K], [K - 1, K], list(range(1, K + 1)), [K // 2, K], [1, K // 2, K - 1, K]):
        edges = sorted(set(edges))
        st = compose(run, seeds, edges)
        got = rs.losses_of(st)
        assert np.array_equal(np.isinf(got), np.isinf(loss)), edges
        np.testing.assert_allclose(got[fin], loss[fin], rtol=1e-9, atol=1e-9, err_msg=str(edges))
        np.testing.assert_allclose(st["z"], zK, rtol=1e-9, atol=1e-9, err_msg=str(edges))
        # the key a segment hands on is gen_k of the forward chain
        k0 = prng.prng_key(seeds)
        _, bb = prng.split(k0)
        c, _ = prng.split(bb)
        _, gen = prng.split(c)
        for _ in range(K):
            _, h = prng.split(gen)
            _, gen = prng.split(h)
        assert np.array_equal(st["key"], gen)


def test_intermediate_gamma_is_the_geometric_bridge_and_the_floor_gives_minus_inf():
    b = synthetic.build("many_gmm_n2000_k256_dds", device="cpu", dense=True, nbridges=4)
    p = synthetic.oracle_params(b["unflatten"], b["params_flat"])
    run = rs.segment_runner(b)
    seeds = synthetic.parity_seeds(200)
    st = run(seeds, 0, 2)
    logp, _ = oracle_target(b["cfg"])(st["z"])
    beta = orc.betas_from_grid(p["mgridref_y"], p["gridref_x"], p["target_x"], np.float64)[1]
    floor = logp == -np.inf
    assert floor.any() and not floor.all()            # init_sigma = 60: some particles sit beyond the -1e4 floor
    assert np.all(st["lg"][floor] == -np.inf) and not np.isnan(st["lg"]).any()
    want = beta * logp[~floor] + (1 - beta) * orc.q_log_prob(p["vd"], st["z"][~floor])
    np.testing.assert_allclose(st["lg"][~floor], want, rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize("name,over", [("gmm_n300_k8", {}), ("many_gmm_n2000_k256_dds", dict(nbridges=8))])
def test_driver_without_resampling_is_the_plain_chain(name, over):
    b = synthetic.build(name, device="cpu", dense=True, **over)
    K = b["params_fixed"][1]
    groups, m = 3, 32
    seeds = synthetic.parity_seeds(groups * m)
    loss, zK = run_oracle(b, seeds)
    out = rs.smc_chain(seeds, rs.segment_runner(b), K, groups=groups, cuts=[1, K // 2, K - 1], ess_threshold=0.0, seed=3)
    assert not out["resampled"].any() and out["resampled"].shape == (3, groups) and out["ess"].shape == (4, groups)
    assert all(np.array_equal(a, np.arange(groups * m)) for a in out["ancestors"])
    fin = np.isfinite(loss)
    assert np.array_equal(np.isinf(out["losses"]), ~fin)
    np.testing.assert_allclose(out["losses"][fin], loss[fin], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(out["z"], zK, rtol=1e-9, atol=1e-9)
    for g in range(groups):
        assert abs(out["ln_Z"][g] - orc.ln_z(loss[g * m:(g + 1) * m])) <= 1e-9


def test_resampled_groups_restart_with_uniform_weights_and_keep_their_keys():
    b = synthetic.build("gmm_n300_k8", device="cpu", dense=True)
    run = rs.segment_runner(b)
    seeds = synthetic.parity_seeds(64)
    st = run(seeds, 0, 4)
    new, trig, ess, inc, anc = rs.resample_stage(st, 2, 1.0, 9)
    assert trig.all() and (ess < 32).all()
    assert np.array_equal(new["key"], st["key"])                      # keys stay with their slot
    assert np.array_equal(new["z"], st["z"][anc]) and np.all(rs.losses_of(new) == 0.0)
    assert (anc[:32] < 32).all() and (anc[32:] >= 32).all()
    for g in range(2):
        assert abs(inc[g] - orc.ln_z(rs.losses_of(st)[g * 32:(g + 1) * 32])) <= 1e-12


def test_the_seeds_of_the_gpu_floor_case_have_the_properties_it_needs():
    import test_gpu_smc as t
    b = synthetic.build("many_gmm_n2000_k256_dds", device="cpu", dense=True, nbridges=8)
    assert b["cfg"]["init_sigma"] == 60.0
    out = rs.smc_chain(t.FLOOR_SEEDS, rs.segment_runner(b), 8, groups=2, cuts=t.FLOOR_CUTS, ess_threshold=1.0, seed=t.FLOOR_RESAMPLE_SEED)
    first = rs.segment_runner(b)(t.FLOOR_SEEDS, 0, t.FLOOR_CUTS[0])
    assert (first["lg"] == -np.inf).any()
    anc = out["ancestors"][0]
    assert np.bincount(anc, minlength=512).max() >= 2
    assert out["resampled"][0].all()


def test_the_seeds_of_the_gpu_unbiasedness_case_pass_with_factor_two():
    import test_gpu_smc as t
    b = synthetic.build(t.UNBIASED_CONFIG, device="cpu", dense=True, **t.UNBIASED_OVER)
    K = b["params_fixed"][1]
    seeds = t.unbiased_seeds()
    out = rs.smc_chain(seeds, rs.segment_runner(b), K, groups=t.UNBIASED_GROUPS, cuts=list(range(1, K)), ess_threshold=0.5,
                       seed=t.UNBIASED_RESAMPLE_SEED)
    zhat = np.exp(out["ln_Z"])
    assert out["resampled"].any()
    assert abs(zhat.mean() - 1.0) <= 2.0 * zhat.std(ddof=1) / np.sqrt(t.UNBIASED_GROUPS), (zhat.mean(), zhat.std(ddof=1))
