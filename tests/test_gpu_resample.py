"""cmcd_amd.resample on the GPU against a float64 NumPy restatement (this module's `restate`: sequential cumulative sum,
np.searchsorted(C, t, side="right"), cmcd_amd/prng.py for the uniforms).  The reference has nothing to compare with.

Two correct scans may round a cumulative boundary differently, so the element-for-element ancestor check is honest only while
no threshold sits on a boundary: every case first asserts, on the CPU, that the restatement's smallest gap min |C_j - t_k|
exceeds 1e-9 (float64 sums of <= 2^20 terms below 1 differ by ~1e-13 at most).  The seeds in CASES were chosen so that every
case passes that guard; none is skipped.

Statistics tolerance: rtol 1e-9 — float64 accumulation over m <= 2^20 terms gives ~m 2^-53 ~ 1e-10, exp / log in double are a
few ulp.  ln Z is also held to utils.log_final_losses with the ln Z bar of tests/helpers.py (1e-3, relative above 1)."""
import functools
import math

import numpy as np
import pytest
import torch

from cmcd_amd import prng, resample, utils

pytestmark = pytest.mark.gpu
CHUNK = resample.CHUNK
GAP = 1e-9
RTOL = 1e-9


# ------------------------------------------------------------------------------------------------ the float64 restatement
def restate(loss, groups, seed):
    """-> (stats[groups, 5] = {n_finite, lnZ, ESS, max weight, diverged}, index[n] global rows, smallest gap |C_j - t_k|)."""
    loss = np.asarray(loss, np.float32)
    n = loss.size
    m = n // groups
    u = prng.uniform(seed, (groups,), 0.0, 1.0)
    stats = np.empty((groups, 5))
    index = np.arange(n, dtype=np.int64)
    gap = math.inf
    for g in range(groups):
        l = loss[g * m:(g + 1) * m].astype(np.float64)
        if np.isnan(l).any() or (l == -np.inf).any():
            stats[g] = [np.nan, np.nan, np.nan, np.nan, 1.0]
            continue
        fin = np.isfinite(l)
        if not fin.any():
            stats[g] = [0.0, -np.inf, 0.0, 0.0, 0.0]
            continue
        M = (-l[fin]).max()
        w = np.exp(-l - M)
        S1, S2 = np.cumsum(w)[-1], np.cumsum(w * w)[-1]
        stats[g] = [fin.sum(), M + math.log(S1) - math.log(m), S1 * S1 / S2, w.max() / S1, 0.0]
        C = np.cumsum(w / S1)
        t = (np.arange(m) + np.float64(u[g])) / m
        a = np.searchsorted(C, t, side="right")
        near = np.minimum(np.abs(C[np.minimum(a, m - 1)] - t), np.abs(C[np.maximum(a - 1, 0)] - t))
        gap = min(gap, float(near.min()))
        index[g * m:(g + 1) * m] = g * m + np.minimum(a, np.flatnonzero(w > 0)[-1])
    return stats, index, gap


# ------------------------------------------------------------------------------------------------ the cases
def make_losses(pattern, m, groups, rng):
    n = m * groups
    if pattern == "equal":
        return np.full(n, 3.25, np.float32)
    if pattern == "dominant":                       # one particle per group 1e4 below the rest
        l = rng.normal(0.0, 1.0, n).astype(np.float32)
        for g in range(groups):
            l[g * m + int(rng.integers(m))] = -1e4
        return l
    if pattern == "heavy":
        return (3.0 * rng.standard_t(2.0, n)).astype(np.float32)
    if pattern == "offset":                         # lgcp-like magnitudes: the shift by the maximum matters
        return (-500.0 + 5.0 * rng.standard_normal(n)).astype(np.float32)
    l = (2.0 * rng.standard_normal(n)).astype(np.float32)
    if pattern == "inf3":                           # the many_gmm floor: ~3 % of the losses +inf
        l[rng.random(n) < 0.03] = np.inf
        l[::m] = np.where(np.isinf(l[::m]), 0.5, l[::m])     # (at least one finite loss per group)
    elif pattern == "allinf":                       # group 1 has no finite loss
        l[m:2 * m] = np.inf
    elif pattern == "diverged":                     # one NaN and one -inf group between healthy neighbours
        l[int(rng.integers(m))] = np.nan                                   # group 0
        l[(groups - 1) * m + int(rng.integers(m))] = -np.inf               # the last group
    else:
        raise KeyError(pattern)
    return l


# (pattern, m, groups, dim, seed): seed feeds the data generator and the resampling call; chosen so that the gap guard holds
CASES = [
    ("heavy", 1, 3, 2, 0), ("heavy", 2, 30, 1, 0), ("heavy", 63, 1, 10, 0), ("heavy", 64, 3, 1, 0), ("heavy", 65, 30, 2, 0),
    ("heavy", CHUNK - 1, 1, 2, 0), ("heavy", CHUNK, 3, 10, 0), ("heavy", CHUNK + 1, 30, 1, 0),
    ("heavy", 2 * CHUNK + 3, 1, 1, 0), ("heavy", 2 * CHUNK + 3, 3, 2, 0), ("heavy", 2 * CHUNK + 3, 30, 10, 0),
    ("heavy", 20, 30, 1600, 0),
    ("equal", 1, 1, 1, 0), ("equal", 65, 3, 2, 0), ("equal", CHUNK + 1, 3, 2, 0), ("equal", 2 * CHUNK + 3, 1, 10, 0),
    ("dominant", 2, 1, 1, 0), ("dominant", 64, 30, 2, 0), ("dominant", CHUNK, 1, 1, 0), ("dominant", 2 * CHUNK + 3, 3, 10, 0),
    ("offset", 63, 30, 10, 0), ("offset", CHUNK - 1, 3, 1, 0), ("offset", 2 * CHUNK + 3, 30, 2, 0),
    ("inf3", 65, 3, 10, 0), ("inf3", CHUNK + 1, 1, 2, 0), ("inf3", 2 * CHUNK + 3, 30, 1, 4),
    ("allinf", 64, 3, 2, 0), ("allinf", CHUNK + 1, 3, 1, 0),
    ("diverged", 65, 30, 2, 0), ("diverged", 2 * CHUNK + 3, 3, 1, 0),
]
IDS = ["%s-m%d-g%d-d%d" % c[:4] for c in CASES]
# determinism, graph replay and the nullable outputs: one case below a chunk, one over several chunks, the wide rows
FEW = [CASES[4], CASES[10], CASES[11], CASES[29]]
FEW_IDS = ["%s-m%d-g%d-d%d" % c[:4] for c in FEW]


@functools.lru_cache(maxsize=None)
def case_data(case):
    """Inputs and the restatement of one case, computed once and shared (read-only) by every test that needs them."""
    pattern, m, groups, dim, seed = case
    rng = np.random.default_rng([seed, m, groups, dim])
    loss = make_losses(pattern, m, groups, rng)
    z = rng.standard_normal((m * groups, dim)).astype(np.float32)
    stats, index, gap = restate(loss, groups, seed)
    for a in (loss, z, stats, index):
        a.setflags(write=False)
    return loss, z, stats, index, gap


def on_device(case):
    loss, z = case_data(case)[:2]
    return torch.from_numpy(loss.copy()).cuda(), torch.from_numpy(z.copy()).cuda()


def stats_matrix(stats):
    return torch.stack([stats[k] for k in resample.STATS], dim=1).cpu().numpy()


def bits(t):
    return t.contiguous().view(torch.int64 if t.element_size() == 8 else torch.int32)


# ------------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_matches_the_float64_restatement(case):
    pattern, m, groups, dim, seed = case
    loss, z, ref_stats, ref_index, gap = case_data(case)
    assert gap > GAP, f"a threshold sits within {gap:.3g} of a cumulative boundary: choose another seed for this case"
    dl, dz = on_device(case)
    out_z, index, stats = resample.resample(dl, dz, groups=groups, seed=seed)
    got = stats_matrix(stats)
    ok = np.isfinite(ref_stats) & (ref_stats != 0)
    print(case, "gap", gap, "max rel stats err", float(np.max(np.abs(got[ok] / ref_stats[ok] - 1.0), initial=0.0)))
    np.testing.assert_allclose(got, ref_stats, rtol=RTOL, atol=0.0, equal_nan=True)
    # ln Z per group against the evaluation's own arithmetic (utils.log_final_losses on that group alone)
    for g in range(groups):
        if ref_stats[g, 4] == 0.0:
            want = utils.log_final_losses(torch.from_numpy(loss[g * m:(g + 1) * m].copy())[None, :])[1]
            have = got[g, 1]
            assert have == want or abs(have - want) <= 1e-3 * max(1.0, abs(want)), (g, have, want)
    assert np.array_equal(index.cpu().numpy().astype(np.int64), ref_index)
    assert out_z.shape == dz.shape and torch.equal(bits(out_z), bits(dz[index.long()]))
    # what the pattern promises
    if pattern == "equal":
        assert np.array_equal(ref_index, np.arange(m * groups)) and np.allclose(got[:, 2], m, rtol=RTOL, atol=0)
    if pattern == "dominant":
        dom = np.flatnonzero(loss == np.float32(-1e4))
        assert np.array_equal(ref_index, np.repeat(dom, m)) and np.allclose(got[:, 2], 1.0, rtol=RTOL, atol=0)
    if pattern == "allinf":
        assert list(got[1]) == [0.0, -np.inf, 0.0, 0.0, 0.0] and np.array_equal(ref_index[m:2 * m], np.arange(m, 2 * m))
    if pattern == "diverged":
        for g in (0, groups - 1):
            assert got[g, 4] == 1.0 and np.isnan(got[g, :4]).all()
            assert np.array_equal(ref_index[g * m:(g + 1) * m], np.arange(g * m, (g + 1) * m))
        assert (got[1:groups - 1, 4] == 0.0).all() and np.isfinite(got[1:groups - 1, :4]).all()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_systematic_scheme_property(case):
    """No restatement in the loop: ancestor j of a non-degenerate group is drawn floor(m W_j) or ceil(m W_j) times, and the
    ancestors do not decrease within a group."""
    pattern, m, groups, dim, seed = case
    loss = case_data(case)[0]
    dl, dz = on_device(case)
    index = resample.launch(dl, None, groups=groups, seed=seed, index=True, copy=False)[1].cpu().numpy().astype(np.int64)
    for g in range(groups):
        l = loss[g * m:(g + 1) * m].astype(np.float64)
        a = index[g * m:(g + 1) * m] - g * m
        assert a.min() >= 0 and a.max() < m and (np.diff(a) >= 0).all()
        if np.isnan(l).any() or (l == -np.inf).any() or not np.isfinite(l).any():
            assert np.array_equal(a, np.arange(m))
            continue
        w = np.exp(-(l - l[np.isfinite(l)].min()))
        mW = m * w / w.sum()
        counts = np.bincount(a, minlength=m)
        assert (counts >= np.floor(mW * (1 - 1e-12))).all() and (counts <= np.ceil(mW * (1 + 1e-12))).all()


@pytest.mark.parametrize("case", FEW, ids=FEW_IDS)
def test_repeated_calls_return_identical_bits(case):
    pattern, m, groups, dim, seed = case
    dl, dz = on_device(case)
    first = resample.resample(dl, dz, groups=groups, seed=seed)
    second = resample.resample(dl, dz, groups=groups, seed=seed)
    assert torch.equal(first[1], second[1]) and torch.equal(bits(first[0]), bits(second[0]))
    for k in resample.STATS:
        assert torch.equal(bits(first[2][k]), bits(second[2][k])), k


@pytest.mark.parametrize("case", FEW, ids=FEW_IDS)
def test_graph_capture_and_replay(case):
    pattern, m, groups, dim, seed = case
    dl, dz = on_device(case)
    eager = resample.resample(dl, dz, groups=groups, seed=seed)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = resample.resample(dl, dz, groups=groups, seed=seed)
    for t in (captured[0], captured[1], *captured[2].values()):
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(eager[1], captured[1]) and torch.equal(bits(eager[0]), bits(captured[0]))
    for k in resample.STATS:
        assert torch.equal(bits(eager[2][k]), bits(captured[2][k])), k


@pytest.mark.parametrize("case", FEW, ids=FEW_IDS)
def test_each_output_alone(case):
    pattern, m, groups, dim, seed = case
    dl, dz = on_device(case)
    both = resample.resample(dl, dz, groups=groups, seed=seed)
    z_none, index, s1 = resample.launch(dl, dz, groups=groups, seed=seed, index=True, copy=False)
    assert z_none is None and torch.equal(index, both[1])
    z_only, index_none, s2 = resample.launch(dl, dz, groups=groups, seed=seed, index=False, copy=True)
    assert index_none is None and torch.equal(bits(z_only), bits(both[0]))
    only = resample.importance_stats(dl, groups=groups)
    for i, k in enumerate(resample.STATS):
        assert torch.equal(bits(only[k]), bits(both[2][k])) and torch.equal(bits(s1[:, i]), bits(s2[:, i])), k


def test_log_importance_diagnostics():
    case = CASES[4]
    m, groups = case[1], case[2]
    ess = case_data(case)[2][:, 2]
    out = utils.log_importance_diagnostics(on_device(case)[0].view(groups, m), log_prefix="_x")
    assert out["ess_x"] == pytest.approx(ess.mean(), rel=1e-9) and out["ess_std_x"] == pytest.approx(ess.std(), rel=1e-9)
    assert out["ess_frac_x"] == pytest.approx(ess.mean() / m, rel=1e-9)
    assert out["ess_frac_std_x"] == pytest.approx(ess.std() / m, rel=1e-9)
