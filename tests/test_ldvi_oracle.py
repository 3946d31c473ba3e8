"""LDVI (`MCD_U_a-lp-sn` / `MCD_U_a-lp`) on the CPU: the restatement tests/ldvi_restatement.py that tests/test_gpu_ldvi.py holds the
HIP path to is pinned here — against an independently written line-by-line NumPy forward (closed-form target scores instead of
autograd), against central finite differences, against the properties the kernels rely on (locality of d / d sn, the network-free
mode at factor_sn = 0) and against ln Z = 0 — together with the case table's claims, the recorded float32 gaps and the host-side
behaviour of cmcd_amd.ldvi that needs no device."""
import math

import numpy as np
import pytest
import torch

import ldvi_cases as lc
import ldvi_restatement as lr
from cmcd_amd import ldvi, model_handler
from cmcd_amd import mcdboundingmachine as mcdbm
from helpers import oracle_target
from oracle import cmcd_oracle as orc
from oracle import prng


def numpy_forward(seeds, p, dim, K, target, use_sn):
    """/root/reference/src/mcdboundingmachine.py:141-179 with mcd_under_lp_a.py:23-87 line by line, float64 NumPy; the target's
    score in closed form (oracle.targets), the grid through np.interp on the two linspaces of mcdboundingmachine.py:113-114."""
    vd = p["vd"]
    e0, rho, n = (a.astype(np.float64) for a in prng.particle_noise_uha(np.asarray(seeds), dim, K))
    G = p["mgridref_y"].shape[0] - 1
    betas = orc.betas_from_grid(p["mgridref_y"], np.linspace(0, 1, G + 2), np.linspace(0, 1, K + 2)[1:-1], np.float64)
    eps, gamma = float(p["eps"]), float(p["gamma"])

    def grad_u(z, beta):                                   # jax.grad(U)(z, beta)                          :18-21
        _, gp = target(z)
        return -1.0 * (beta * gp + (1.0 - beta) * orc.q_grad(vd, z))

    z = orc.q_sample(vd, e0)                               # mcdboundingmachine.py:156
    w = -orc.q_log_prob(vd, z)                             # :157
    w = w - orc.log_prob_kernel(rho, np.zeros_like(rho), 1.0)   # mcd_under_lp_a.py:70-71
    for i in range(K):
        beta = betas[i]
        eta_aux = gamma * eps                              # :28
        fk_rho_mean = rho * (1.0 - eta_aux)                # :29
        scale = np.sqrt(2.0 * eta_aux)                     # :30
        rho_prime = fk_rho_mean + scale * n[:, i, :]       # :33
        rho_prime_prime = rho_prime - eps * grad_u(z, beta) / 2.0          # :35
        z_new = z + eps * rho_prime_prime                  # :36
        rho_new = rho_prime_prime - eps * grad_u(z_new, beta) / 2.0        # :37
        if not use_sn:
            bk_rho_mean = rho_prime * (1.0 - eta_aux)      # :41
        else:
            input_sn = np.concatenate([z, rho_prime], 1)   # :48
            bk_rho_mean = rho_prime * (1.0 - eta_aux) + 2 * eta_aux * orc.apply_geffner(p["sn"], input_sn, i, np.float64)
        fk_log_prob = orc.log_prob_kernel(rho_prime, fk_rho_mean, scale)   # :54
        bk_log_prob = orc.log_prob_kernel(rho, bk_rho_mean, scale)         # :55
        w = w + (bk_log_prob - fk_log_prob)                # :58
        z, rho = z_new, rho_new
    w = w + orc.log_prob_kernel(rho, np.zeros_like(rho), 1.0)   # :85
    w = w + target(z)[0]                                   # mcdboundingmachine.py:178
    return -1.0 * w, z


@pytest.mark.parametrize("case_id", sorted(lc.CASES))
def test_restatement_agrees_with_the_numpy_forward(case_id):
    p, (dim, K, mode, _), model = lc.params_of(case_id)
    seeds = lc.seeds_of(case_id)
    l, z = lr.forward(seeds, p, dim, K, model, use_sn=mode == "MCD_U_a-lp-sn")
    l_np, z_np = numpy_forward(seeds, p, dim, K, oracle_target(lc.build(case_id)["cfg"]), mode == "MCD_U_a-lp-sn")
    assert np.array_equal(np.isinf(l), np.isinf(l_np))
    f = np.isfinite(l)
    assert np.abs(l[f] - l_np[f]).max() <= 1e-11 * max(1.0, np.abs(l_np[f]).max())
    assert np.abs(z - z_np).max() <= 1e-12 * max(1.0, np.abs(z_np).max())
    # the gradient call of the restatement returns the same forward values
    l_g, z_g, _ = lc.reference(case_id)
    assert np.array_equal(l_g[f], l[f]) and np.array_equal(z_g, z)


def _mean_loss(p, seeds, dim, K, model):
    return float(np.mean(lr.forward(seeds, p, dim, K, model)[0]))


@pytest.mark.parametrize("path,index,h", [(("eps",), (), 1e-6), (("gamma",), (), 1e-4), (("mgridref_y",), (3,), 1e-5),
                                          (("vd", "logdiag"), (1,), 1e-6), (("vd", "mean"), (0,), 1e-6),
                                          (("sn", "factor_sn"), (), 1e-6), (("sn", "W1"), (2, 5), 1e-5)])
def test_autograd_agrees_with_central_differences(path, index, h):
    """float64, gmm K = 8, seeds 1 .. 17: d mean(loss) / d one entry of eps, gamma, mgridref_y, vd, factor_sn and W1."""
    import copy
    p, (dim, K, _, _), model = lc.params_of("gmm-n17")
    seeds = lc.seeds_of("gmm-n17")
    _, _, g = lr.bound_and_grad(seeds, p, dim, K, model)
    got = g
    for k in path:
        got = got[k]
    got = float(np.asarray(got)[index])
    vals = []
    for sgn in (+1.0, -1.0):
        q = copy.deepcopy(p)
        leaf = q
        for k in path[:-1]:
            leaf = leaf[k]
        a = np.array(leaf[path[-1]], np.float64)
        a[index] += sgn * h
        leaf[path[-1]] = a
        vals.append(_mean_loss(q, seeds, dim, K, model))
    fd = (vals[0] - vals[1]) / (2 * h)
    assert abs(got - fd) <= 1e-6 * max(1.0, abs(fd)), (path, got, fd)
    assert got != 0.0


def test_eta_is_not_read():
    """The tree's eta leaf (mcdboundingmachine.py:60-63) is unused by this mode: zero gradient."""
    _, _, g = lc.reference("gmm-n17")
    b = lc.build("gmm-n17")
    off = b["unflatten"].offset("eta")
    assert off >= 0 and float(g[off]) == 0.0


def test_factor_zero_gives_the_network_free_mode_exactly():
    import copy
    p, (dim, K, _, _), model = lc.params_of("gmm-n33")
    seeds = lc.seeds_of("gmm-n33")
    q = copy.deepcopy(p)
    q["sn"]["factor_sn"] = np.zeros(())
    l_sn, z_sn = lr.forward(seeds, q, dim, K, model, use_sn=True)
    l_no, z_no = lr.forward(seeds, q, dim, K, model, use_sn=False)
    assert np.array_equal(l_sn, l_no) and np.array_equal(z_sn, z_no)
    l_on, z_on = lr.forward(seeds, p, dim, K, model, use_sn=True)
    assert np.array_equal(z_on, z_no)                    # the positions never depend on the network
    assert np.abs(l_on - l_no).max() > 1e-3              # ... the weights do


@pytest.mark.parametrize("case_id", ["gmm-n17", "funnel"])
def test_sn_gradient_is_local(case_id):
    """d / d sn from full autograd equals the one from the cotangent -omega (rho - m_b) on s with the trajectory detached:
    what ldvi_net_grad_kernel computes per (particle, bridge)."""
    p, (dim, K, _, _), model = lc.params_of(case_id)
    seeds = lc.seeds_of(case_id)
    _, _, g = lr.bound_and_grad(seeds, p, dim, K, model)
    _, _, g_loc = lr.bound_and_grad(seeds, p, dim, K, model, local_sn=True)
    for k in lr.SN_LEAVES:
        m = np.abs(g["sn"][k]).max()
        assert m > 0 and np.abs(g["sn"][k] - g_loc["sn"][k]).max() <= 1e-12 * m, k


def test_ln_z_of_gmm_is_zero_within_sampling_error():
    """logmeanexp(-loss) estimates ln Z = 0 of the normalised gmm without bias in Z: a few thousand seeds, three standard errors
    (delta method on the weights).  A q that covers the three modes and 16 bridges: weights of moderate spread."""
    dim = 2
    flat, un, fixed = ldvi.initialize(dim, vdparams={"mean": torch.zeros(2), "logdiag": torch.full((2,), math.log(3.0))},
                                      nbridges=16, eps=0.1, gamma=5.0, emb_dim=20, mode="MCD_U_a-lp", nn_arch="geffner",
                                      device="cpu")
    p = lr.params_numpy(un, flat)
    seeds = np.arange(1, 4001, dtype=np.int32)
    l, _ = lr.forward(seeds, p, dim, 16, "gmm", use_sn=False)
    wts = np.exp(-l)
    se = wts.std(ddof=1) / math.sqrt(len(wts)) / wts.mean()
    assert se < 0.1, se
    assert abs(math.log(wts.mean())) <= 3 * se, (math.log(wts.mean()), se)
    assert np.mean(-l) < math.log(wts.mean())            # the ELBO lies below ln Z


# ------------------------------------------------------------------------------------------ the case table
def test_case_table_claims():
    # tiles and workgroups of the gmm sizes (16 particles per tile, four tiles per workgroup of the sweep)
    tiles = {n: (n + 15) // 16 for n in (1, 16, 17, 33, 65)}
    assert tiles == {1: 1, 16: 1, 17: 2, 33: 3, 65: 5} and (tiles[65] + 3) // 4 == 2 and 65 % 16 == 1 and 17 % 16 == 1
    # widths: 2 d + emb on 16-neuron tiles
    for cid, width, T in (("gmm-n33", 24, 2), ("funnel", 68, 5), ("many-floor", 24, 2)):
        dim, K, _, spec = lc.build(cid)["params_fixed"]
        assert 2 * dim + spec.emb_dim == width and (width + 15) // 16 == T and spec.rho_dim == dim and spec.arch == "geffner"
    assert lc.build("nonet")["params_fixed"][3] is None
    # K = 40 on the 33-node grid: non-uniform, fractions inside (0, 1), cells with two bridges
    p, (dim, K, _, _), _ = lc.params_of("gmm-k40")
    m = p["mgridref_y"]
    assert K == 40 and m.shape == (33,) and np.ptp(m) > 0.5
    pos = np.arange(1, K + 1) / (K + 1) * 33
    frac, cell = pos - np.floor(pos), np.floor(pos).astype(int)
    assert ((frac > 0.01) & (frac < 0.99)).all() and np.bincount(cell).max() == 2
    assert lc.params_of("gmm-k1")[1][1] == 1
    # every trainable leaf of every case has a non-zero reference gradient, eta excepted
    for cid in lc.CASES:
        b = lc.build(cid)
        _, _, g = lc.reference(cid)
        for name, (e, s) in lr.block_errors(b["unflatten"], g, g).items():
            assert (s == 0.0) == (name == "eta"), (cid, name)


def test_floor_case_claims():
    """Seeds from 1 .. 64 by the band guard: at least 32 kept, at least 4 floored, at least 16 finite; and float32 does not take
    any kept evaluation across the floor (the guard's reason)."""
    seeds, l_all, lp = lc.floor_scan()
    keep = lc.seeds_of("many-floor")
    m = np.isin(seeds, keep)
    assert (np.abs(lp[:, m] - lc.FLOOR) > lc.BAND).all()
    l, _, _ = lc.reference("many-floor")
    assert len(keep) >= 32 and int(np.isinf(l).sum()) >= 4 and int(np.isfinite(l).sum()) >= 16
    assert np.array_equal(np.isinf(l), lp[-1, m] <= lc.FLOOR) and (l[np.isinf(l)] > 0).all()
    p, (dim, K, _, _), model = lc.params_of("many-floor")
    trace = {}
    lr.forward(keep, p, dim, K, model, trace=trace, dtype=torch.float32)
    assert np.abs(np.stack(trace["lp"]) - lp[:, m]).max() <= lc.BAND / 10


# ------------------------------------------------------------------------------------------ the cases past the first ten
MAX_SLABS = 512      # kLdviMaxSlabs of cmcd_amd/csrc/cmcd_ldvi.hip: the item kernel's workgroups = slabs of partials

# id: (tiles, items, {items per slab: slabs})
SLAB_CLAIMS = {
    "gmm-slabs": (13, 520, {2: 8, 1: 504}),
    "gmm-slabs-k33": (17, 561, {2: 49, 1: 463}),
    "funnel-slabs": (9, 576, {2: 64, 1: 448}),
    "gmm-nw4": (1025, 1025, {3: 1, 2: 511}),
    "gmm-nw8": (8193, 8193, {17: 1, 16: 511}),
}
# id: (width, its own tile count, the instance it runs on)
WIDTH_CLAIMS = {
    "gmm-w29": (33, 3, 4), "gmm-w44": (44, 3, 4), "gmm-w64": (64, 4, 4), "many-w64": (64, 4, 4),
    "funnel-w65": (65, 5, 5), "funnel-w80": (80, 5, 5), "funnel-slabs": (68, 5, 5), "funnel-n65": (68, 5, 5),
    "gmm-slabs": (24, 2, 2), "many-n33": (24, 2, 2),
}
# id: (waves per forward workgroup, forward workgroups, live waves of the last one)
WAVE_CLAIMS = {"gmm-slabs": (1, 13, 1), "gmm-nw4": (4, 257, 1), "gmm-nw8": (8, 1025, 1)}
NEW_CASES = ("gmm-slabs", "gmm-slabs-k33", "funnel-slabs", "gmm-w29", "gmm-w44", "gmm-w64", "many-w64", "funnel-w65", "funnel-w80",
             "funnel-n1", "funnel-n16", "funnel-n65", "many-n33", "funnel-nonet", "many-nonet", "gmm-nw4", "gmm-nw8")
EARLIER_CASES = ("funnel", "gmm-k1", "gmm-k40", "gmm-n1", "gmm-n16", "gmm-n17", "gmm-n33", "gmm-n65", "many-floor", "nonet")


def _tiles(case_id):
    return (len(lc.seeds_of(case_id)) + 15) // 16


def _slab_walk(items):
    """-> (nslabs, the items each workgroup walks: b, b + nslabs, ..)."""
    nslabs = min(items, MAX_SLABS)
    return nslabs, [list(range(b, items, nslabs)) for b in range(nslabs)]


def _instance(dim, T):
    """The neuron tiles of the instance a width of T tiles runs on (cmcd_api.hip: hidden_width; cmcd_ldvi.hip: ldvi_traj_pick)."""
    padded = 2 if T <= 2 else (4 if T <= 4 else (5 if T <= 5 else None))      # hidden_width's rounding
    return padded if padded in {2: (2, 4), 10: (5,)}[dim] else None         # the instances ldvi_traj_pick has for this dimension


def _nw(tiles):
    return 1 if tiles <= 1024 else (4 if tiles <= 8192 else 8)     # ldvi_launch


def test_the_table_is_the_ten_earlier_cases_and_the_seventeen_new_ones():
    assert sorted(lc.CASES) == sorted(NEW_CASES + EARLIER_CASES) and len(NEW_CASES) == 17
    # the largest item count of the earlier ten is 80: every workgroup of theirs handles one item
    assert max(_tiles(c) * lc.params_of(c)[1][1] for c in EARLIER_CASES) == 80
    expect_n = {"gmm-slabs": 208, "gmm-slabs-k33": 257, "funnel-slabs": 129, "gmm-w29": 17, "gmm-w44": 17, "gmm-w64": 17,
                "funnel-w65": 17, "funnel-w80": 17, "funnel-n1": 1, "funnel-n16": 16, "funnel-n65": 65, "funnel-nonet": 17,
                "gmm-nw4": 16400, "gmm-nw8": 131088}
    for cid, n in expect_n.items():
        assert np.array_equal(lc.seeds_of(cid), np.arange(1, n + 1)), cid
    expect_k = {"gmm-slabs": 40, "gmm-slabs-k33": 33, "funnel-slabs": 64, "many-w64": 8, "funnel-w65": 4, "funnel-w80": 4,
                "funnel-n1": 4, "funnel-n16": 4, "funnel-n65": 4, "many-n33": 8, "funnel-nonet": 4, "many-nonet": 8, "gmm-nw4": 1,
                "gmm-nw8": 1, "gmm-w29": 8, "gmm-w44": 8, "gmm-w64": 8}
    for cid, K in expect_k.items():
        assert lc.params_of(cid)[1][1] == K, cid
    # gmm-slabs and gmm-k40 are the same parameters (the in-between call of the GPU test runs both)
    assert torch.equal(lc.build("gmm-slabs")["params_flat"], lc.build("gmm-k40")["params_flat"])
    # the funnel's n- and width-cases are the funnel case's parameters but for the width
    for cid in ("funnel-n1", "funnel-n16", "funnel-n65"):
        assert torch.equal(lc.build(cid)["params_flat"], lc.build("funnel")["params_flat"])
    for cid in ("funnel", "funnel-w65", "funnel-w80", "funnel-nonet"):
        p = lc.params_of(cid)[0]
        assert float(p["eps"]) == np.float32(0.05) and float(p["gamma"]) == 4.0, cid
    for cid in ("many-w64", "many-n33", "many-nonet"):
        p = lc.params_of(cid)[0]
        assert float(p["eps"]) == np.float32(0.05) and float(p["gamma"]) == 2.0, cid
        assert np.allclose(np.exp(p["vd"]["logdiag"]).mean(), 60.0, rtol=0.3)      # the configuration's sigma, not many-floor's 100


@pytest.mark.parametrize("case_id", sorted(SLAB_CLAIMS))
def test_slab_walk_claims(case_id):
    tiles, items, per_slab = SLAB_CLAIMS[case_id]
    K = lc.params_of(case_id)[1][1]
    assert _tiles(case_id) == tiles and K * tiles == items
    nslabs, walk = _slab_walk(items)
    assert nslabs == MAX_SLABS < items and sorted(sum(walk, [])) == list(range(items))
    count = {}
    for w in walk:
        count[len(w)] = count.get(len(w), 0) + 1
    assert count == per_slab
    n = len(lc.seeds_of(case_id))
    split = [[(item // tiles, item % tiles) for item in w] for w in walk]      # (bridge, tile) of the item kernel
    if case_id == "gmm-slabs":
        # both the bridge and the tile change inside every walk of two: 512 = 39 x 13 + 5
        assert all(a[0] != b[0] and a[1] != b[1] for a, b in (s for s in split if len(s) == 2))
    if case_id in ("gmm-slabs-k33", "funnel-slabs"):
        # the last tile holds one particle, and it is the second item of some slabs and the only item of others
        assert n % 16 == 1 and MAX_SLABS % tiles != 0
        second = [s for s in split if len(s) == 2 and s[1][1] == tiles - 1]
        assert len(second) == {"gmm-slabs-k33": 3, "funnel-slabs": 8}[case_id]
        assert any(len(s) == 1 and s[0][1] == tiles - 1 for s in split)
    if case_id.startswith("gmm-nw"):
        assert K == 1 and all(b == 0 for s in split for b, _ in s)


@pytest.mark.parametrize("case_id", sorted(WIDTH_CLAIMS))
def test_width_claims(case_id):
    width, T, inst = WIDTH_CLAIMS[case_id]
    dim, K, _, spec = lc.build(case_id)["params_fixed"]
    assert 2 * dim + spec.emb_dim == width and (width + 15) // 16 == T and _instance(dim, T) == inst
    assert spec.rho_dim == dim and spec.arch == "geffner"
    pad = 16 * inst - width
    assert pad == {"gmm-w29": 31, "gmm-w44": 20, "gmm-w64": 0, "many-w64": 0, "funnel-w65": 15, "funnel-w80": 0}.get(case_id, pad)
    if case_id == "gmm-w29":
        assert width - 32 == 1            # one unit in the third tile, the fourth all padding
    if case_id == "gmm-w44":
        assert T == 3 and inst == 4       # a whole padded tile
    if case_id == "funnel-w65":
        assert width - 64 == 1            # one unit in the fifth tile


def test_network_free_claims():
    for cid, model, dim, K in (("funnel-nonet", "funnel", 10, 4), ("many-nonet", "many_gmm", 2, 8)):
        b = lc.build(cid)
        assert b["params_fixed"] == (dim, K, "MCD_U_a-lp", None) and b["cfg"]["model"] == model
        assert b["unflatten"].offset("sn", "emb") == -1 and b["unflatten"].offset("gamma") >= 0


@pytest.mark.parametrize("case_id", sorted(WAVE_CLAIMS))
def test_forward_wave_claims(case_id):
    nw, groups, live = WAVE_CLAIMS[case_id]
    tiles = _tiles(case_id)
    assert _nw(tiles) == nw and (tiles + nw - 1) // nw == groups and tiles - (groups - 1) * nw == live
    if nw > 1:
        assert _nw(tiles - 1) < nw        # the smallest tile count of this rule, hence the smallest n
        assert len(lc.seeds_of(case_id)) == 16 * (tiles - 1) + 16


def test_sweep_workgroup_claims():
    """Four tiles per workgroup of the sweep: funnel-n65 opens a second one with one live wave; n = 1 and 16 are one tile."""
    assert _tiles("funnel-n1") == 1 and _tiles("funnel-n16") == 1 and 16 % 16 == 0
    assert _tiles("funnel-n65") == 5 and (5 + 3) // 4 == 2 and 5 - 4 == 1 and 65 % 16 == 1


@pytest.mark.parametrize("case_id", ["many-w64", "many-n33", "many-nonet"])
def test_band_guard_of_the_ordinary_many_gmm_cases(case_id):
    """Seeds from 1 .. 40 by the band guard: what is kept (all 40 here: three tiles), that a kept floored particle sits far past
    the floor, and that float32 takes no kept evaluation across it."""
    seeds, l_all, lp = lc.floor_scan(case_id)
    assert np.array_equal(seeds, np.arange(1, 41))
    keep = lc.seeds_of(case_id)
    m = np.isin(seeds, keep)
    assert np.array_equal(m, (np.abs(lp - lc.FLOOR) > lc.BAND).all(0))
    assert len(keep) == 40 and len(keep) >= 17
    l, _, _ = lc.reference(case_id)
    floored = np.isinf(l)
    assert np.array_equal(floored, lp[-1, m] <= lc.FLOOR) and int(floored.sum()) == 1 and (l[floored] > 0).all()
    assert (lp[-1, m][floored] < lc.FLOOR - lc.BAND).all()
    # away from the floor regime: many-floor floors at least 4 of its 64
    assert int(np.isfinite(l).sum()) == 39
    p, (dim, K, mode, _), model = lc.params_of(case_id)
    trace = {}
    lr.forward(keep, p, dim, K, model, use_sn=mode == "MCD_U_a-lp-sn", trace=trace, dtype=torch.float32)
    lp32 = np.stack(trace["lp"])
    assert np.array_equal(lp32 <= lc.FLOOR, lp[:, m] <= lc.FLOOR)
    assert np.abs(lp32 - lp[:, m]).max() <= lc.BAND / 10


def test_float32_gaps_are_the_recorded_ones():
    """tests/golden/ldvi_gaps.json (python tests/ldvi_cases.py --write) holds, per case, what float32 alone costs the restatement:
    the worst particle's loss and every gradient block over its own maximum.  The device's bar of a block is
    max(2e-3, 4 x the record); re-measured here: never above a quarter of that bar, and the losses far inside compare_losses'."""
    stored = lc.stored_gaps()
    assert set(stored) == set(lc.CASES)
    for cid in lc.CASES:
        gap = lc.float32_gap(cid)
        assert gap["loss"] <= 2.5e-4, (cid, gap["loss"])           # a quarter of compare_losses' worst-particle bar (K <= 32)
        assert set(gap["blocks"]) == set(stored[cid]["blocks"]), cid
        for name, g in gap["blocks"].items():
            assert g <= lc.bar_of(cid, name) / 4.0, (cid, name, g, stored[cid]["blocks"][name])


# ------------------------------------------------------------------------------------------ host side, no device
def test_initialize_returns_the_second_order_tree():
    kw = dict(nbridges=8, eps=0.02, gamma=7.0, eta=0.3, emb_dim=20, nlayers=3, seed=5, nn_arch="geffner", device="cpu",
              trainable=("eta", "gamma", "eps", "vd", "mgridref_y"))
    flat, un, fixed = ldvi.initialize(2, mode="MCD_U_a-lp-sn", **kw)
    flat2, un2, fixed2 = mcdbm.initialize(2, mode="MCD_CAIS_UHA_sn", **kw)
    assert torch.equal(flat, flat2) and un.layout == un2.layout
    assert fixed == (2, 8, "MCD_U_a-lp-sn", fixed2[3]) and fixed2[3].rho_dim == 2
    flat3, un3, fixed3 = ldvi.initialize(2, mode="MCD_U_a-lp", **kw)
    assert fixed3 == (2, 8, "MCD_U_a-lp", None) and un3.offset("sn", "emb") == -1 and un3.offset("gamma") >= 0
    assert ldvi.MODES == ("MCD_U_a-lp-sn", "MCD_U_a-lp")
    with pytest.raises(NotImplementedError, match="nn_arch"):
        ldvi.initialize(2, mode="MCD_U_a-lp-sn", **dict(kw, nn_arch="dds"))
    with pytest.raises(NotImplementedError, match="Mode not implemented"):
        ldvi.initialize(2, mode="MCD_U_a-lp-sna", **kw)
    with pytest.raises(NotImplementedError):                # the bounding machine itself still refuses the mode
        mcdbm.initialize(2, mode="MCD_U_a-lp-sn", **kw)


def test_validation_order_on_cpu_tensors():
    """mode, target type, target dim, then the device — the order of the other entry points."""
    b = lc.build("gmm-n17")
    flat, un, fixed, tgt = b["params_flat"], b["unflatten"], b["params_fixed"], b["target"]
    seeds = torch.arange(1, 5, dtype=torch.int32)
    funnel = model_handler.load_model("funnel")[0]
    for fn in (ldvi.bound_forward, ldvi.compute_bound, ldvi.grad_and_loss):
        with pytest.raises(NotImplementedError, match="Mode not implemented"):
            fn(seeds, flat, un, (2, 8, "MCD_U_ea-lp-sn", fixed[3]), object())
        with pytest.raises(TypeError, match="model_handler.Target"):
            fn(seeds, flat, un, fixed, lambda z: z)
        with pytest.raises(ValueError, match="target dim"):
            fn(seeds, flat, un, fixed, funnel)
        with pytest.raises(RuntimeError, match="ROCm device"):
            fn(seeds, flat, un, fixed, tgt)
    dds = fixed[3]._replace(arch="dds")
    with pytest.raises(NotImplementedError, match="nn_arch"):
        ldvi.bound_forward(seeds, flat, un, (2, 8, "MCD_U_a-lp-sn", dds), tgt)
