"""CPU checks of the mean-field VI restatement (oracle.cmcd_oracle.mfvi_*): consistency with the
nbridges = 0 limit of the MCD restatement and the closed-form gradient against finite differences; and of the cases of
tests/mfvi_cases.py: that each is what it is there for (record counts and their remainder modulo four, the floor cases' category
counts under the two seed guards, identical +inf sets at float32 and float64, floor-all's closed-form gradient) and that the
restatement's own float32 gap is at most a quarter of the bar tests/test_gpu_mfvi.py holds the kernels to.

A floored particle (many_gmm: log p <= -1e4 becomes -inf) follows the convention otg.ManyGmm already returns, grad log p = 0 with
the -1 of d / d logdiag kept: the `jnp.where` of the reference's src/model_handler.py:279-280 differentiates its constant branch."""
import numpy as np
import pytest

from oracle import cmcd_oracle as orc
from oracle import targets as otg

import gated_cases as gc
import mfvi_cases as mc
import trained_cases as tc
from helpers import lgcp_counts_fixture


def _target(name):
    if name == "gmm":
        return otg.Gmm(), 2
    if name == "funnel":
        return otg.Funnel(10), 10
    if name == "many_gmm":
        return otg.ManyGmm(), 2
    return otg.Lgcp(lgcp_counts_fixture()), 1600


def _vd(name, dim):
    rng = np.random.default_rng(3)
    if name == "lgcp":
        return {"mean": np.full(dim, np.log(126.0) - 0.955) + 0.05 * rng.standard_normal(dim),
                "logdiag": np.full(dim, np.log(0.5)) + 0.05 * rng.standard_normal(dim)}
    sig = 15.0 if name == "many_gmm" else 1.0
    return {"mean": 0.3 * rng.standard_normal(dim), "logdiag": np.log(sig) + 0.1 * rng.standard_normal(dim)}


@pytest.mark.parametrize("name", ["gmm", "funnel", "many_gmm"])
def test_mfvi_is_the_zero_bridge_limit(name):
    """boundingmachine.compute_log_elbo with nbridges = 0 and the MCD machine with no steps draw the same z
    from the same key and add the same two terms."""
    target, dim = _target(name)
    vd = _vd(name, dim)
    seeds = np.arange(1, 40, dtype=np.int32)
    l, z = orc.mfvi_losses(seeds, vd, dim, target)
    p = {"vd": vd, "eps": np.float64(0.1), "mgridref_y": np.ones(1), "gridref_x": np.linspace(0, 1, 2),
         "target_x": np.zeros(0)}
    l2, z2 = orc.compute_log_elbo_batch(seeds, p, dim, 0, "MCD_ULA", "dds", target, dtype=np.float64)
    np.testing.assert_array_equal(z, z2)
    np.testing.assert_allclose(l, l2, rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize("name", ["gmm", "funnel", "many_gmm", "lgcp"])
def test_mfvi_gradient_matches_finite_differences(name):
    target, dim = _target(name)
    vd = _vd(name, dim)
    seeds = np.arange(1, 13 if name == "lgcp" else 65, dtype=np.int32)
    g = orc.mfvi_grad(seeds, vd, dim, target)
    rng = np.random.default_rng(0)
    coords = range(dim) if dim <= 10 else rng.choice(dim, 5, replace=False)
    h = 1e-5
    for leaf in ("mean", "logdiag"):
        for j in coords:
            vp = {k: v.copy() for k, v in vd.items()}
            vm = {k: v.copy() for k, v in vd.items()}
            vp[leaf][j] += h
            vm[leaf][j] -= h
            fd = (orc.mfvi_losses(seeds, vp, dim, target)[0].mean() - orc.mfvi_losses(seeds, vm, dim, target)[0].mean()) / (2 * h)
            assert abs(fd - g[leaf][j]) <= 1e-6 * max(1.0, abs(fd)), (leaf, j, fd, g[leaf][j])


# ------------------------------------------------------------------------------------------ the cases of tests/mfvi_cases.py
def test_case_list_is_the_one_the_gpu_tests_expect():
    assert len(set(mc.IDS)) == len(mc.IDS) == 34
    for cid in ("gmm-145", "funnel-133", "lgcp-65", "lgcp-33", "floor-half", "floor-all", "trained-many-dds"):
        assert cid in mc.IDS
    assert sorted(c[0][len("trained-"):] for c in mc.CASES if c[3]["kind"] == "trained") == sorted(tc.TRAINED_ROWS)


@pytest.mark.parametrize("name", ["gmm", "funnel", "many_gmm", "lgcp"])
def test_setup_q_is_the_q_of_the_existing_tests(name):
    """{"kind": "setup"} is `_vd` above (and test_gpu_mfvi._setup), rounded to the float32 the device receives."""
    q = mc.q_of(("x", name, 1, mc.SETUP, {}))
    for k, v in _vd(name, mc.dim_of(name)).items():
        assert q[k].dtype == np.float32 and np.array_equal(q[k], v.astype(np.float32))


def test_every_remainder_of_the_four_wide_reduction_is_reached():
    """mfvi_reduce_kernel sums `count` rows four at a time plus a remainder loop; the five cases before these had count % 4 in
    {1, 3} only.  Each case's `records` is what the issue states for it; the tile path and lgcp each reach remainder 0."""
    seen = {"tile": set(), "lgcp": set()}
    for case in mc.CASES:
        count = mc.records_of(case)
        n = len(mc.seeds_of(case))
        assert count == (n if case[1] == "lgcp" else -(-n // 16))
        if "records" in case[4]:
            assert count == case[4]["records"], case[0]
        seen["lgcp" if case[1] == "lgcp" else "tile"].add(count % 4)
    assert seen["tile"] == {0, 1, 2, 3} and seen["lgcp"] >= {0, 1}, seen
    by = {c[0]: mc.records_of(c) for c in mc.CASES}
    assert by["gmm-64"] % 4 == 0 and by["gmm-96"] % 4 == 2 and by["gmm-33"] % 4 == 3 and by["funnel-133"] % 4 == 1
    assert by["lgcp-32"] % 4 == 0 and by["lgcp-257"] == 257
    # passes of the lgcp loop: one, one full, two, three, nine
    assert [-(-by[c] // mc.LGCP_PASS) for c in ("lgcp-1", "lgcp-32", "lgcp-33", "lgcp-65", "lgcp-257")] == [1, 1, 2, 3, 9]
    # the tile path's 145 particles: ten tiles in three workgroups of four waves, the last with two idle
    assert by["gmm-145"] == 10 and -(-10 // 4) == 3 and 3 * 4 - 10 == 2


@pytest.mark.parametrize("cid", [c[0] for c in mc.CASES if not mc.is_floor(c)])
def test_plain_cases_are_finite(cid):
    l, z, g = mc.reference(mc.case_by_id(cid))
    assert np.isfinite(l).all() and np.isfinite(z).all() and all(np.isfinite(v).all() for v in g.values())


@pytest.mark.parametrize("cid", [c[0] for c in mc.CASES if mc.is_floor(c)])
def test_floor_cases_are_what_they_say(cid):
    """Category counts and the two guards' drop counts (conditions of the issue, not measurements): no case loses more than
    5 % of its seeds, floor-half keeps >= 30 floored and >= 30 unfloored particles, floor-sparse (and the trained sigma = 60
    row) >= 2 floored; every floor case but floor-all has a tile with both kinds, floor-all's three tiles hold +inf
    losses only.  A floored particle's loss is +inf and nothing else is."""
    case = mc.case_by_id(cid)
    rep = mc.guard_report(case)
    extras = case[4]
    print(cid, rep)
    assert rep["near"] + rep["ridge"] <= mc.MAX_DROP * rep["n0"], rep
    assert rep["floored"] >= extras.get("min_floored", 0) and rep["unfloored"] >= extras.get("min_unfloored", 0), rep
    l, z, _ = mc.reference(case)
    otarget = mc.oracle_side(case)[0]
    lp = otarget.unfloored(z)
    assert np.array_equal(np.isinf(l), lp <= gc.FLOOR) and not np.isnan(l).any() and (l[np.isinf(l)] > 0).all()
    assert int(np.isinf(l).sum()) == rep["floored"]
    assert (np.abs(lp - gc.FLOOR) > gc.DELTA * -gc.FLOOR).all()
    deep = (lp > gc.FLOOR) & (lp < mc.DEEP)
    assert (gc.component_gap(z[deep]) >= gc.RIDGE_NATS).all()
    tiles = [np.isinf(l[i:i + 16]) for i in range(0, len(l), 16)]
    if extras.get("all_floored"):
        assert rep["unfloored"] == 0 and rep["kept"] == rep["n0"] == 33 and all(t.all() for t in tiles)
    else:
        assert any(t.any() and not t.all() for t in tiles), "no tile with finite and +inf losses"
    if cid in ("floor-sparse", "trained-many-dds"):
        assert rep == dict(n0=145, near=0, ridge=0, kept=145, floored=3, unfloored=142)


def test_the_trained_sigma_60_row_is_the_floor_sparse_q():
    """train_vi is off on that row: its snapshot's q is the reference's initial many_gmm q, mean 0 and sigma 60."""
    a, b = mc.q_of(mc.case_by_id("trained-many-dds")), mc.q_of(mc.case_by_id("floor-sparse"))
    assert all(np.array_equal(a[k], b[k]) for k in a)


def test_floored_particles_keep_the_minus_one():
    """The convention for a floored particle is what otg.ManyGmm returns, grad log p = 0 (the `jnp.where` of the reference's
    src/model_handler.py:279-280 differentiates the constant branch), so `mfvi_grad` gives d / d mean = 0 and
    d / d logdiag = -1 for it: floor-all's gradient in closed form, at float64 and float32; and in a mixed batch the gradient
    is the finite particles' sum plus -1 per floored particle on logdiag, over n."""
    case = mc.case_by_id("floor-all")
    otarget, dim, vd = mc.oracle_side(case)
    for dt in (np.float64, np.float32):
        g = orc.mfvi_grad(mc.seeds_of(case), vd, dim, otarget, dtype=dt)
        assert np.array_equal(g["mean"], np.zeros(2)) and np.array_equal(g["logdiag"], -np.ones(2))
    case = mc.case_by_id("floor-half")
    otarget, dim, vd = mc.oracle_side(case)
    seeds = mc.seeds_of(case)
    l, _, g = mc.reference(case)
    f = np.isfinite(l)
    gf = orc.mfvi_grad(seeds[f], vd, dim, otarget)
    n, nf = len(seeds), int(f.sum())
    np.testing.assert_allclose(g["mean"], gf["mean"] * nf / n, rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(g["logdiag"], (gf["logdiag"] * nf - (n - nf)) / n, rtol=1e-12, atol=1e-15)
    assert np.isfinite(g["mean"]).all() and np.isfinite(g["logdiag"]).all() and np.isinf(l.mean())


@pytest.mark.parametrize("cid", mc.IDS)
def test_float32_gap_is_within_a_quarter_of_the_bar(cid):
    """The restatement's own float32 run (identical +inf set, asserted by float32_gap) against float64: each metric's gap is
    at most trained_cases.QUARTER of the bar tests/test_gpu_mfvi.py holds the kernel to, max(1e-4, FACTOR x gap); and the
    gaps stay where the issue measured them (1.4e-5 on a loss, 5.5e-5 at sd 1e-4, 8.7e-6 on a leaf), 1.5 x at most."""
    case = mc.case_by_id(cid)
    gl, gg = mc.float32_gap(case)
    bl, bg = mc.bars(case)
    print(cid, gl, gg, bl, bg)
    assert tc.FACTOR * tc.QUARTER == 1.0
    assert gl <= tc.QUARTER * bl and all(gg[k] <= tc.QUARTER * bg[k] for k in gg)
    assert gl <= 1.5 * (5.5e-5 if cid == "gmm-narrow-1e-4" else 1.4e-5)
    assert max(gg.values()) <= 1.5 * 8.7e-6
    if cid != "gmm-narrow-1e-4":
        assert bl == mc.FLOOR_BAR
    assert all(b == mc.FLOOR_BAR for b in bg.values())
