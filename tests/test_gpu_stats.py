"""The five on-device statistics `stats[5] = {n_finite, sum l, sum l^2, max(-l), sum exp(-l - max)}` (float64) of every
kernel form, pinned to float64: every per-tile record writer through every merge it can reach (the fused last-arriver merge
of grids of <= 64 workgroups, the finalize launch), on batches that hold the edges — +inf particles, tiles of +inf
particles only, ragged last tiles, tiles whose maximum lies thousands of nats below the batch's — and the merges alone
(finalize_kernel through cmcd_stats_merge_device, the host cmcd_stats_merge, the torch-op merge of parallel.merge_stats) on
records no forward call produces.  The reference is oracle.cmcd_oracle.stats5 on the losses the device returned
(helpers.check_stats; DESIGN.md section 2, "Statistics contract")."""
import math

import numpy as np
import pytest
import torch

from cmcd_amd import _lib
from cmcd_amd import mcdboundingmachine as mcdbm
from cmcd_amd import parallel, synthetic
from oracle import cmcd_oracle as orc

from helpers import check_stats, lgcp_counts_fixture, run_oracle

gpu = pytest.mark.gpu

TRAJ, COOP16, COOP8 = "traj_kernel", "coop_kernel<16-particle tiles>", "coop_kernel<8-particle tiles>"
KERNEL = {1: TRAJ, 2: COOP8, 3: COOP16, 4: COOP8}       # many_gmm / gmm, batches of <= 2048 particles (2: the library's tile)
TILE = {1: 16, 2: 8, 3: 16, 4: 8}
ALL_INF = [0.0, math.inf, math.inf, -math.inf, 0.0]
WORST = {}                                              # observed worst errors per sum, relative to their scale (printed per case)


def _check(stats, losses, tag):
    rep = check_stats(stats, losses, tag)
    for k in ("rel_sum", "rel_sumsq", "rel_exp", "lnz_err"):
        WORST[k] = max(WORST.get(k, 0.0), rep[k])
    print("STATS", tag, {k: (f"{v:.2e}" if isinstance(v, float) else v) for k, v in rep.items()}, "worst so far",
          {k: f"{v:.2e}" for k, v in WORST.items()})
    return rep


# ------------------------------------------------------------------------------------------ inputs that hold the edges
_BUILT, _POOL, _ORACLE = {}, {}, {}
POOL_CFG = ("many_gmm_n2000_k256_dds", dict(nbridges=4))        # init_sigma = 60: particles beyond the floor of log p


def _build(name, dense=False, **over):
    key = (name, dense, tuple(sorted(over.items())))
    if key not in _BUILT:
        kw = dict(over)
        if name.startswith("lgcp"):
            kw["lgcp_counts"] = lgcp_counts_fixture()
        _BUILT[key] = synthetic.build(name, device="cuda", dense=dense, **kw)
    return _BUILT[key]


def _oracle_inf(name, seeds, **over):
    """+inf set of the float64 oracle on `seeds`, once per (configuration, seeds)."""
    key = (name, tuple(sorted(over.items())), seeds.tobytes())
    if key not in _ORACLE:
        b = synthetic.build(name, device="cpu", dense=False, **over)
        _ORACLE[key] = np.isinf(run_oracle(b, seeds, dtype=np.float64)[0])
    return _ORACLE[key]


def _pool():
    """4096 seeds of the headline target at K = 4 by their float64-oracle class: 196 +inf, finite losses from -5 to 10 792
    (exp(max_tile - max_batch) underflows to zero for whole tiles).  One oracle run per module."""
    if not _POOL:
        seeds = synthetic.parity_seeds(4096)
        inf = _oracle_inf(POOL_CFG[0], seeds, **POOL_CFG[1])
        _POOL.update(seeds=seeds, inf=inf, i_inf=np.flatnonzero(inf), i_fin=np.flatnonzero(~inf))
        assert len(_POOL["i_inf"]) >= 40 and len(_POOL["i_fin"]) >= 2048
    return _POOL


def _batch(kind, n, tile=16):
    """-> (seeds[n], oracle +inf mask[n]).  Indices wrap round the pool for n > 4096 (a seed may repeat in a batch)."""
    p = _pool()
    nat = np.arange(2 * 4096) % 4096
    if kind == "mixed":             # natural order, from the first window that holds both classes
        start = 0
        while not (p["inf"][nat[start:start + n]].any() and not p["inf"][nat[start:start + n]].all()):
            start += 1
        idx = nat[start:start + n]
    elif kind == "finite":
        idx = p["i_fin"][np.arange(n) % len(p["i_fin"])]
    elif kind == "all_inf":
        idx = p["i_inf"][np.arange(n) % len(p["i_inf"])]
    elif kind == "inf_first":       # the first 16 seeds +inf: an 8-particle and a 16-particle tile of +inf only
        head = p["i_inf"][:16]
        rest = nat[~np.isin(nat, head)]
        idx = np.concatenate([head, rest])[:n]
        assert n > 16 and p["inf"][idx[:16]].all() and not p["inf"][idx[16:]].all()
    elif kind == "inf_last":        # n = tile m + 3, the ragged last tile holds +inf only
        assert n % tile == 3
        tail = p["i_inf"][-3:]
        rest = nat[~np.isin(nat, tail)]
        idx = np.concatenate([rest[:n - 3], tail])
        assert p["inf"][idx[-3:]].all() and not p["inf"][idx[:-3]].all()
    else:
        raise KeyError(kind)
    return p["seeds"][idx], p["inf"][idx]


def _forward(b, seeds, variant, monkeypatch):
    monkeypatch.setattr(mcdbm, "KERNEL_VARIANT", variant)
    losses, z, stats = mcdbm.bound_forward(torch.from_numpy(np.ascontiguousarray(seeds)).cuda(), b["params_flat"], b["unflatten"],
                                           b["params_fixed"], b["target"], eps_schedule=b["eps_schedule"],
                                           grad_clipping=b["grad_clipping"])
    torch.cuda.synchronize()
    return losses, stats, _lib.last_kernel_name()


def _edge_case(variant, kind, n, monkeypatch, records=None):
    """One forward call of the headline target on an edge batch: the kernel form, the record count, the batch's property,
    the device's +inf set against the oracle's, then the statistics."""
    tile = TILE[variant]
    seeds, inf = _batch(kind, n, tile)
    b = _build(POOL_CFG[0], **POOL_CFG[1])
    losses, stats, kernel = _forward(b, seeds, variant, monkeypatch)
    assert kernel == KERNEL[variant], kernel
    if records is not None:
        assert -(-n // tile) == records
    lh = losses.double().cpu().numpy()
    assert np.array_equal(np.isinf(lh), inf), f"+inf set differs from the oracle's at {np.flatnonzero(np.isinf(lh) != inf)}"
    assert not np.isnan(lh).any()
    if kind == "finite":
        assert not inf.any()
    elif kind == "all_inf":
        assert inf.all()
    else:
        assert inf.any() and not inf.all()
    if kind == "inf_first":
        assert inf[:16].all()
    if kind == "inf_last":
        assert inf[-3:].all() and n % tile == 3
    _check(stats, losses, f"variant {variant} {kind} n={n}")
    return losses, stats


# ------------------------------------------------------------------------------------------ many_gmm: the three tilings
# wave per tile: 4081 = 255 tiles + 1, 4097 = 257 records (256 -> 257: finalize_kernel's threads go from one record to two)
@gpu
@pytest.mark.parametrize("kind,n", [("mixed", 16), ("mixed", 17), ("mixed", 4081), ("mixed", 4097), ("inf_first", 17),
                                    ("inf_first", 4081), ("inf_first", 4097), ("inf_last", 19), ("inf_last", 4083),
                                    ("inf_last", 4099), ("finite", 1), ("all_inf", 1), ("finite", 4097)])
def test_wave_per_tile_records_through_finalize(hip_lib, monkeypatch, kind, n):
    _edge_case(1, kind, n, monkeypatch, records={4081: 256, 4083: 256, 4097: 257, 4099: 257}.get(n))


# 16-particle tiles: 64 records = the fused merge by the last workgroup, 65 = the finalize launch
@gpu
@pytest.mark.parametrize("kind,n,records", [("mixed", 1024, 64), ("mixed", 1025, 65), ("inf_first", 1024, 64),
                                            ("inf_first", 1025, 65), ("inf_last", 1011, 64), ("inf_last", 1027, 65),
                                            ("finite", 1024, 64), ("finite", 1025, 65), ("finite", 1, 1), ("all_inf", 1, 1)])
def test_cooperative_16_particle_records_fused_and_finalize(hip_lib, monkeypatch, kind, n, records):
    _edge_case(3, kind, n, monkeypatch, records=records)


# 8-particle tiles (2: the library's choice for <= 2048 particles, 4: forced)
@gpu
@pytest.mark.parametrize("variant", [2, 4])
@pytest.mark.parametrize("kind,n,records", [("mixed", 9, 2), ("mixed", 512, 64), ("mixed", 513, 65), ("mixed", 2041, 256),
                                            ("inf_first", 512, 64), ("inf_first", 513, 65), ("inf_first", 2041, 256),
                                            ("inf_last", 11, 2), ("inf_last", 507, 64), ("inf_last", 515, 65),
                                            ("inf_last", 2043, 256), ("finite", 512, 64), ("finite", 513, 65)])
def test_cooperative_8_particle_records_fused_and_finalize(hip_lib, monkeypatch, variant, kind, n, records):
    _edge_case(variant, kind, n, monkeypatch, records=records)


@gpu
@pytest.mark.parametrize("variant", [1, 2, 3, 4])
@pytest.mark.parametrize("n", [40, 196, 520])
def test_a_batch_of_inf_particles_only(hip_lib, monkeypatch, variant, n):
    """Every record is {0, inf, inf, -inf, 0}: the merged statistics too, bit for bit; compute_bound returns +inf,
    compute_bound_var NaN (inf - inf, like the reference's var), ln Z = -inf."""
    losses, stats = _edge_case(variant, "all_inf", n, monkeypatch)
    assert stats.cpu().tolist() == ALL_INF
    b = _build(POOL_CFG[0], **POOL_CFG[1])
    seeds = torch.from_numpy(_batch("all_inf", n)[0]).cuda()
    kw = dict(eps_schedule=b["eps_schedule"], grad_clipping=b["grad_clipping"])
    mean, (l2, _) = mcdbm.compute_bound(seeds, b["params_flat"], b["unflatten"], b["params_fixed"], b["target"], **kw)
    var, _ = mcdbm.compute_bound_var(seeds, b["params_flat"], b["unflatten"], b["params_fixed"], b["target"], **kw)
    assert torch.equal(l2, losses) and float(mean) == math.inf and math.isnan(float(var))
    assert float(mcdbm.ln_z_from_stats(stats, n)) == -math.inf and float(parallel.finalize(stats, n)["ln_z"]) == -math.inf


@gpu
@pytest.mark.parametrize("variant,n", [(1, 4081), (3, 1025), (3, 1024), (2, 513), (4, 512), (4, 2041)])
@pytest.mark.parametrize("kind", ["mixed", "finite"])
def test_statistics_do_not_depend_on_the_batch_composition(hip_lib, monkeypatch, variant, n, kind):
    """The same particles in another order (the +inf ones in other tiles): n_finite and the maximum bit for bit, the three
    sums within the bound of any summation order (both calls pass check_stats on the same multiset of losses)."""
    seeds, inf = _batch(kind, n)
    perm = np.random.default_rng(n).permutation(n)
    tiles = lambda mask: set((np.flatnonzero(mask) // TILE[variant]).tolist())
    assert kind == "finite" or tiles(inf) != tiles(inf[perm])
    b = _build(POOL_CFG[0], **POOL_CFG[1])
    la, sa, ka = _forward(b, seeds, variant, monkeypatch)
    lb, sb, kb = _forward(b, seeds[perm], variant, monkeypatch)
    assert ka == kb == KERNEL[variant]
    assert torch.equal(lb.cpu(), la.cpu()[perm])
    assert (kind == "mixed") == bool(torch.isinf(la).any())
    ra = _check(sa, la, f"composition {variant} {kind} n={n}")
    rb = _check(sb, lb, f"composition {variant} {kind} n={n} permuted")
    assert ra["n_inf"] == rb["n_inf"] == int(inf.sum())
    a, c = sa.cpu().numpy(), sb.cpu().numpy()
    assert a[0] == c[0] and a[3] == c[3]
    if kind == "mixed":
        assert a[1] == c[1] == np.inf and a[2] == c[2] == np.inf


# ------------------------------------------------------------------------------------------ the other record writers
@gpu
@pytest.mark.parametrize("mode", ["MCD_CAIS_var_sn", "MCD_CAIS_sn"])
@pytest.mark.parametrize("variant", [1, 2, 3, 4])
@pytest.mark.parametrize("n", [203, 520])
def test_the_132_wide_instances(hip_lib, monkeypatch, mode, variant, n):
    """The 132-wide geffner net on many_gmm (the VarGrad configuration) at sigma_0 = 60: the tail4 wave-per-tile instance and
    the 12-wave cooperative instances with the merged RNG / ACC wave (the MERGE record writer); 8-particle tiles: 26 records
    (fused merge) and 65 (finalize), 16-particle tiles: 13 and 33 (fused)."""
    over = dict(nbridges=4, init_sigma=60.0, boundmode=mode)
    b = _build("many_gmm_var_n16000_k256", **over)
    seeds = synthetic.parity_seeds(n)
    inf = _oracle_inf("many_gmm_var_n16000_k256", synthetic.parity_seeds(520), **over)[:n]
    losses, stats, kernel = _forward(b, seeds, variant, monkeypatch)
    assert kernel == (TRAJ if variant == 1 else f"coop_kernel<{TILE[variant]}-particle tiles, 132-wide net>"), kernel
    assert -(-n // TILE[variant]) == {(203, 8): 26, (520, 8): 65, (203, 16): 13, (520, 16): 33}[(n, TILE[variant])]
    assert inf.any() and np.array_equal(torch.isinf(losses).cpu().numpy(), inf)
    _check(stats, losses, f"132-wide {mode} variant {variant} n={n}")


@gpu
@pytest.mark.parametrize("variant", [4, 5, 3, 1])
@pytest.mark.parametrize("n", [300, 513, 520])
def test_funnel_records(hip_lib, param_set, monkeypatch, variant, n):
    """d = 10: coop_wide8_kernel (4), coop_kernel on 8-particle tiles (5) and on 16-particle tiles (3), wave per tile (1);
    8-particle tiles: 38 records (fused merge), 65 (finalize)."""
    b = _build("funnel_n300_k64", dense=param_set == "dense", nbridges=3)
    losses, stats, kernel = _forward(b, synthetic.parity_seeds(n), variant, monkeypatch)
    assert kernel == {4: "coop_wide8_kernel<8-particle tiles>", 5: COOP8, 3: COOP16, 1: TRAJ}[variant], kernel
    assert torch.isfinite(losses).all()
    _check(stats, losses, f"funnel variant {variant} n={n}")


@gpu
@pytest.mark.parametrize("variant", [1, 2, 3])
@pytest.mark.parametrize("n", [1, 300])
def test_gmm_records(hip_lib, param_set, monkeypatch, variant, n):
    b = _build("gmm_n300_k8", dense=param_set == "dense", nbridges=3)
    losses, stats, kernel = _forward(b, synthetic.parity_seeds(n), variant, monkeypatch)
    assert kernel == KERNEL[variant], kernel
    _check(stats, losses, f"gmm variant {variant} n={n}")


UHA = "MCD_CAIS_UHA_sn"
UHA_KERNEL = {1: "uha_traj_kernel", 3: "uha_coop_kernel<16-particle tiles>", 4: "uha_coop_kernel<8-particle tiles>",
              5: "uha_coop_kernel<8-particle tiles>"}


@gpu
@pytest.mark.parametrize("variant,n", [(1, 1500), (3, 1500), (3, 1024), (4, 1500), (4, 512)])
def test_second_order_records_on_a_mixed_batch(hip_lib, monkeypatch, variant, n):
    """2nd-order CMCD (cmcd_uha.hip: its own record writers, the finalize launch): many_gmm at sigma_0 = 60, +inf particles."""
    over = dict(nbridges=4, boundmode=UHA, init_eps=0.2, init_gamma=2.0)
    b = _build("many_gmm_n2000_k256_dds", **over)
    inf = _oracle_inf("many_gmm_n2000_k256_dds", synthetic.parity_seeds(1500), **over)[:n]
    losses, stats, kernel = _forward(b, synthetic.parity_seeds(n), variant, monkeypatch)
    assert kernel == UHA_KERNEL[variant], kernel
    assert inf.any() and np.array_equal(torch.isinf(losses).cpu().numpy(), inf)
    _check(stats, losses, f"2nd-order variant {variant} n={n}")


@gpu
@pytest.mark.parametrize("variant", [4, 5])
@pytest.mark.parametrize("n", [77, 300])
def test_second_order_funnel_on_8_particle_tiles(hip_lib, param_set, monkeypatch, variant, n):
    """The funnel's 8-particle form with the tail wave (4) and without (5)."""
    b = _build("funnel_n300_k64", dense=param_set == "dense", nbridges=3, boundmode=UHA, init_eps=0.05, init_gamma=4.0)
    losses, stats, kernel = _forward(b, synthetic.parity_seeds(n), variant, monkeypatch)
    assert kernel == UHA_KERNEL[variant], kernel
    _check(stats, losses, f"2nd-order funnel variant {variant} n={n}")


@gpu
@pytest.mark.parametrize("n,variant,mode,kernel", [
    (5, 0, "MCD_CAIS_sn", "lgcp launch sequence"), (17, 0, "MCD_CAIS_sn", "lgcp launch sequence"),
    (40, 0, "MCD_CAIS_sn", "lgcp launch sequence"),                 # two passes of 32 rows
    (230, 0, "MCD_CAIS_sn", "lgcp wide-batch"),                     # the wide-batch form by the library's choice
    (20, 3, "MCD_CAIS_sn", "lgcp launch sequence"),                 # the split-K sequence
    (257, 2, "MCD_CAIS_sn", "lgcp wide-batch"),                     # wide, forced: 256 -> 257 records
    (20, 0, UHA, "lgcp launch sequence"),                           # the 2nd-order sequence
    (33, 3, UHA, "lgcp launch sequence")])                          # ... its split-K form: records per pass at partials + base * CMCD_NSTATS
def test_lgcp_records(hip_lib, monkeypatch, n, variant, mode, kernel):
    """d = 1600, K = 2: one record per particle; losses of magnitude 1e3 .. 1e4 — the hard case for the sum of squares."""
    over = dict(nbridges=2, boundmode=mode, **(dict(init_eps=0.02, init_gamma=5.0) if mode == UHA else {}))
    b = _build("lgcp_n20_k128", **over)
    losses, stats, name = _forward(b, synthetic.parity_seeds(n), variant, monkeypatch)
    assert name.startswith(kernel), name
    assert torch.isfinite(losses).all()
    _check(stats, losses, f"lgcp {mode} variant {variant} n={n}")


@gpu
@pytest.mark.parametrize("model,n", [("gmm", 300), ("funnel", 301), ("many_gmm", 2000), ("many_gmm", 7), ("lgcp", 29)])
def test_mean_field_records(hip_lib, model, n):
    """cmcd_mfvi.hip's record writer, with and without the gradient."""
    from cmcd_amd import boundingmachine as bm
    from test_gpu_mfvi import _setup
    target, _, dim, flat, unflatten, fixed, _ = _setup(model, n)
    seeds = torch.from_numpy(synthetic.parity_seeds(n)).cuda()
    for want_grad in (False, True):
        _, losses, _, stats = bm._call(seeds, flat, unflatten, fixed, target, want_grad)
        torch.cuda.synchronize()
        _check(stats, losses, f"mean-field {model} n={n} grad={want_grad}")


# ------------------------------------------------------------------------------------------ the gradient entry points
@gpu
@pytest.mark.parametrize("item", ["0", "1"], ids=["whole_chain", "work_items"])
@pytest.mark.parametrize("name,n", [("many_gmm_n2000_k256_dds", 203), ("gmm_n300_k8", 33)])
def test_statistics_of_the_gradient_entry_points(hip_lib, monkeypatch, name, n, item):
    """compute_bound_grad(return_stats=True) and compute_log_var_grad (its statistics: what it hands to `stats_total`) return
    the statistics of the losses they return; a +inf particle in a VarGrad batch gives an all-NaN gradient (jax.grad of a NaN
    variance)."""
    monkeypatch.setenv("CMCD_GRAD_ITEM", item)
    many = name.startswith("many")
    seeds = _batch("finite", n)[0] if many else synthetic.parity_seeds(n)
    b = _build(name, nbridges=4)
    kw = dict(eps_schedule=b["eps_schedule"], grad_clipping=b["grad_clipping"])
    grad, (losses, _), stats = mcdbm.compute_bound_grad(torch.from_numpy(seeds).cuda(), b["params_flat"], b["unflatten"],
                                                        b["params_fixed"], b["target"], return_stats=True, **kw)
    torch.cuda.synchronize()
    assert torch.isfinite(losses).all() and torch.isfinite(grad).all()
    _check(stats, losses, f"compute_bound_grad {name} item {item}")

    bv = _build(name, nbridges=4, boundmode="MCD_CAIS_var_sn")
    seen = []

    def keep(local):
        seen.append(local.clone())
        return local
    batches = [("finite", seeds)] + ([("mixed", _batch("mixed", n)[0])] if many else [])
    reached = None
    for kind, sd in batches:
        inf = _oracle_inf(name, sd, nbridges=4, boundmode="MCD_CAIS_var_sn")
        grad, (losses, _) = mcdbm.compute_log_var_grad(torch.from_numpy(sd).cuda(), bv["params_flat"], bv["unflatten"],
                                                       bv["params_fixed"], bv["target"], stats_total=keep, **kw)
        torch.cuda.synchronize()
        assert np.array_equal(torch.isinf(losses).cpu().numpy(), inf)
        _check(seen[-1], losses, f"compute_log_var_grad {name} {kind} item {item}")
        if kind == "finite":
            assert not inf.any() and torch.isfinite(grad).all()
            reached = grad != 0          # the leaves the loss reaches (jax.grad gives an exact zero for the others)
            assert reached.sum() > 1000
        else:
            assert inf.any() and torch.isnan(grad[reached]).all() and not torch.isinf(grad).any()
            assert (torch.isnan(grad) | (grad == 0)).all()


# ------------------------------------------------------------------------------------------ the merges alone
COUNTS = [1, 2, 255, 256, 257, 1000, 15000]            # 15 000: the record count of the reference's lgcp evaluation batch
PATTERNS = ["empty_rows", "one_row_only", "inf_rows", "all_inf", "spread_maxima", "equal_maxima", "maximum_in_last_row", "huge"]
EMPTY = np.array([0.0, 0.0, 0.0, -np.inf, 0.0])


def _rows(pattern, count):
    """-> (rows [count, 5] of oracle stats5 per contiguous part, n per part, all losses)."""
    rng = np.random.default_rng(count * 31 + PATTERNS.index(pattern))
    sizes = rng.integers(1, 4, count)
    if pattern == "empty_rows":             # empty parts at the front, in the middle and at the end
        for lo, hi in ((0, max(1, count // 10)), (count // 2, count // 2 + max(1, count // 7)), (count - max(1, count // 9), count)):
            sizes[lo:hi] = 0
        if not sizes.any():
            sizes[count // 3] = 2
    elif pattern == "one_row_only":
        sizes[:] = 0
        sizes[(2 * count) // 3] = 5
    parts = []
    top = int(rng.integers(0, count))
    for r, m in enumerate(sizes):
        l = rng.normal(3.0, 2.0, m)
        if pattern in ("empty_rows", "inf_rows") and m and r % 5 == 1:
            l[0] = np.inf
        if pattern == "inf_rows" and r % 3 == 0:
            l[:] = np.inf
        elif pattern == "all_inf":
            l[:] = np.inf
        elif pattern == "spread_maxima":    # maxima over +-2000: most rescales underflow, row `top` dominates
            l += rng.uniform(-2000.0, 2000.0) if r != top else -2100.0
        elif pattern == "equal_maxima":
            l[:] = np.abs(l)
            l[0] = -5.0
        elif pattern == "maximum_in_last_row":
            l[:] = np.abs(l)
            if r == count - 1:
                l[-1] = -40.0
        elif pattern == "huge":             # sum of squares ~ 1e36: beyond a float32 accumulator
            l[:] = rng.choice([-1e18, 1e18], m) * rng.uniform(0.5, 1.0, m)
        parts.append(l)
    rows = np.array([orc.stats5(p) if len(p) else EMPTY for p in parts])
    return rows, sizes, np.concatenate(parts)


def _host_merges(rows, sizes):
    merged, mean, var, lnz = _lib.stats_merge(rows.tolist(), sizes.tolist())
    return np.array(merged), parallel.merge_stats(torch.from_numpy(rows)).numpy()


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("count", COUNTS)
def test_host_merges_against_stats5_of_the_whole(hip_lib, pattern, count):
    """cmcd_stats_merge and the torch-op merge of parallel.merge_stats (no device): both within check_stats of the whole
    batch; n_finite and the maximum bit-equal between them."""
    rows, sizes, whole = _rows(pattern, count)
    c_merge, torch_merge = _host_merges(rows, sizes)
    check_stats(c_merge, whole, f"cmcd_stats_merge {pattern} x{count}")
    check_stats(torch_merge, whole, f"torch-op merge {pattern} x{count}")
    assert c_merge[0] == torch_merge[0] and c_merge[3] == torch_merge[3]
    if pattern == "all_inf":
        assert c_merge.tolist() == ALL_INF and torch_merge.tolist() == ALL_INF


@gpu
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("count", COUNTS)
def test_finalize_kernel_on_caller_rows(hip_lib, pattern, count):
    """cmcd_stats_merge_device = finalize_kernel on the caller's rows, against stats5 of the whole and the two host merges."""
    rows, sizes, whole = _rows(pattern, count)
    dev = parallel.merge_stats(torch.from_numpy(rows).cuda()).cpu().numpy()
    c_merge, torch_merge = _host_merges(rows, sizes)
    _check(dev, whole, f"finalize_kernel {pattern} x{count}")
    check_stats(c_merge, whole, f"cmcd_stats_merge {pattern} x{count}")
    check_stats(torch_merge, whole, f"torch-op merge {pattern} x{count}")
    assert dev[0] == c_merge[0] == torch_merge[0] and dev[3] == c_merge[3] == torch_merge[3]
    if pattern == "all_inf":
        assert dev.tolist() == ALL_INF


def _rows_with_an_infinite_maximum(count):
    """Integer-valued losses (every sum exact in any order), one part with a -inf loss: its record has max = +inf, and so has
    the merged one — every other record's exp-sum is dropped, the +inf-maximum records' passes through unscaled."""
    rng = np.random.default_rng(count)
    parts = [rng.integers(-3, 9, int(m)).astype(np.float64) for m in rng.integers(0, 4, count)]
    hit = count // 2
    parts[hit] = np.array([2.0, -np.inf, 1.0])
    rows = np.array([orc.stats5(p) if len(p) else EMPTY for p in parts])
    assert rows[hit, 3] == np.inf
    rows[hit, 4] = 1.0              # (stats5 gives 0 here; a non-zero value shows whether the merge passes it through)
    if count > 4:
        rows[count - 1] = [1.0, -np.inf, np.inf, np.inf, 2.0]
    return rows, np.array([max(1, len(p)) for p in parts])


def _assert_same_merge(a, b, count):
    want4 = 3.0 if count > 4 else 1.0
    for k in range(5):
        assert a[k] == b[k], (k, a, b)
    assert a[1] == -np.inf and a[2] == np.inf and a[3] == np.inf and a[4] == want4


@pytest.mark.parametrize("count", [1, 2, 257, 1000])
def test_host_merges_agree_on_an_infinite_maximum(hip_lib, count):
    rows, sizes = _rows_with_an_infinite_maximum(count)
    c_merge, torch_merge = _host_merges(rows, sizes)
    _assert_same_merge(c_merge, torch_merge, count)


@gpu
@pytest.mark.parametrize("count", [1, 2, 257, 1000])
def test_finalize_kernel_agrees_on_an_infinite_maximum(hip_lib, count):
    rows, sizes = _rows_with_an_infinite_maximum(count)
    dev = parallel.merge_stats(torch.from_numpy(rows).cuda()).cpu().numpy()
    c_merge, torch_merge = _host_merges(rows, sizes)
    _assert_same_merge(dev, c_merge, count)
    _assert_same_merge(dev, torch_merge, count)
