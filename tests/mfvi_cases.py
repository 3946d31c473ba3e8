"""Cases of the mean-field call (cmcd_amd.boundingmachine over cmcd_mfvi_bound_grad: cmcd_mfvi.hip, and lgcp_mfvi /
lgcp_mfvi_finish_kernel of cmcd_lgcp.hip), shared by tests/test_oracle_mfvi.py (which asserts on the CPU, from the float64
restatement alone, that each case is what it says) and tests/test_gpu_mfvi.py (the HIP path against oracle.cmcd_oracle.mfvi_*).

A case is `(id, model, n, q, extras)`:
  q       how the mean-field q is made (`q_of`): {"kind": "setup"} draws it as test_gpu_mfvi._setup does (default_rng(3); lgcp: sd
          0.5 or `sd`; many_gmm: sigma 15; `logdiag0` replaces the first log std); {"kind": "fixed", "mean", "sd"} is that q
          exactly; {"kind": "trained", "id"} takes the vd leaves of tests/golden/trained_<id>.npz;
  extras  n_mixes (many_gmm components, 40 when absent), records (the records the reduction must see; test_oracle_mfvi.py
          re-derives it), floor (a case with +inf losses, whose seeds pass the two guards below), min_floored / min_unfloored.
Seeds are synthetic.parity_seeds(n); for a floor case the survivors of parity_seeds(n) under the guards.

What each shape is there for, read against the kernels.  The tile path writes one record and one gradient row per 16-particle
tile, four tiles per workgroup, and mfvi_reduce_kernel sums the rows four at a time plus a remainder: n = 1 (one lane), 16 (a
full tile), 17 (one particle in a second tile whose 15 invalid lanes read seeds[n - 1] and must add nothing), 33 (3 records),
64 (4: the unrolled loop alone), 96 (6: remainder 2), 145 (10 tiles: three workgroups, two idle waves).  lgcp writes one record
and one row per particle in passes of kMP = 32: n = 32 is one full pass, 33 and 65 start a second and third on the workspace
the first left, 257 is nine passes and takes the finalize launch from 256 to 257 records.  many_gmm with 7, 17 and 64
components runs the kernel's inline staging loop off its usual bound.  The floor cases put -inf into log p (many_gmm's floor at
-1e4): the particle's gradient of log p is 0, the -1 of d / d logdiag stays, its loss is +inf beside a finite gradient.
"""
import functools
import types

import numpy as np
import torch

import gated_cases as gc
import trained_cases as tc
from cmcd_amd import synthetic
from oracle import cmcd_oracle as orc
from oracle import targets as otg

from helpers import lgcp_counts_fixture

SETUP = {"kind": "setup"}
FLOOR_N0 = 145
MAX_DROP = 0.05                 # share of a case's n0 seeds the guards may take
DEEP = -2000.0                  # the ridge guard looks at unfloored particles below this many nats

CASES = [
    # ---- tile path: batch edges and record counts
    ("gmm-1", "gmm", 1, SETUP, dict(records=1)),
    ("gmm-16", "gmm", 16, SETUP, dict(records=1)),
    ("gmm-17", "gmm", 17, SETUP, dict(records=2)),
    ("gmm-33", "gmm", 33, SETUP, dict(records=3)),
    ("gmm-64", "gmm", 64, SETUP, dict(records=4)),
    ("gmm-96", "gmm", 96, SETUP, dict(records=6)),
    ("gmm-145", "gmm", 145, SETUP, dict(records=10)),
    ("funnel-5", "funnel", 5, SETUP, dict(records=1)),
    ("funnel-21", "funnel", 21, SETUP, dict(records=2)),
    ("funnel-133", "funnel", 133, SETUP, dict(records=9)),
    # ---- many_gmm off its 40 components
    ("many-mix7", "many_gmm", 49, SETUP, dict(n_mixes=7, records=4)),
    ("many-mix17", "many_gmm", 49, SETUP, dict(n_mixes=17, records=4)),
    ("many-mix64", "many_gmm", 49, SETUP, dict(n_mixes=64, records=4)),
] + [
    # ---- the q of the trained snapshots (many-dds: the sigma = 60 row, three floored particles)
    ("trained-" + cid, row["model"], 145, {"kind": "trained", "id": cid}, dict(floor=True, min_floored=2) if cid == "many-dds" else {})
    for cid, row in tc.TRAINED_ROWS.items()
] + [
    # ---- narrow and wide q
    ("gmm-narrow-1e-2", "gmm", 145, {"kind": "fixed", "mean": (3.0, -2.0), "sd": 1e-2}, {}),
    ("gmm-narrow-1e-4", "gmm", 145, {"kind": "fixed", "mean": (3.0, -2.0), "sd": 1e-4}, {}),
    ("funnel-wide", "funnel", 133, {"kind": "setup", "logdiag0": float(np.log(3.0))}, {}),
    # ---- the floor
    ("floor-sparse", "many_gmm", FLOOR_N0, {"kind": "fixed", "mean": (0.0, 0.0), "sd": 60.0}, dict(floor=True, min_floored=2)),
    ("floor-half", "many_gmm", FLOOR_N0, {"kind": "fixed", "mean": (110.0, 110.0), "sd": 15.0},
     dict(floor=True, min_floored=30, min_unfloored=30)),
    ("floor-all", "many_gmm", 33, {"kind": "fixed", "mean": (300.0, 300.0), "sd": 1.0}, dict(floor=True, all_floored=True, records=3)),
    # ---- lgcp: passes of 32
    ("lgcp-1", "lgcp", 1, SETUP, dict(records=1)),
    ("lgcp-32", "lgcp", 32, SETUP, dict(records=32)),
    ("lgcp-33", "lgcp", 33, SETUP, dict(records=33)),
    ("lgcp-65", "lgcp", 65, SETUP, dict(records=65)),
    ("lgcp-257", "lgcp", 257, SETUP, dict(records=257)),
    ("lgcp-sd0.1", "lgcp", 33, {"kind": "setup", "sd": 0.1}, {}),
    ("lgcp-sd2", "lgcp", 33, {"kind": "setup", "sd": 2.0}, {}),
]
IDS = [c[0] for c in CASES]
LGCP_PASS = 32                  # kMP of cmcd_lgcp.hip


def case_by_id(cid):
    return next(c for c in CASES if c[0] == cid)


def is_floor(case):
    return bool(case[4].get("floor"))


def dim_of(model):
    return {"gmm": 2, "funnel": 10, "many_gmm": 2, "lgcp": 1600}[model]


def q_of(case):
    """-> {"mean", "logdiag"} float32 arrays: the q the device receives (the oracle takes the same values as float64)."""
    _, model, _, q, _ = case
    dim = dim_of(model)
    if q["kind"] == "trained":
        leaves = tc.load_fixture(q["id"])[1]
        mean, logdiag = leaves[("vd", "mean")], leaves[("vd", "logdiag")]
        assert mean.shape == logdiag.shape == (dim,)
    elif q["kind"] == "fixed":
        mean = np.asarray(q["mean"], np.float64)
        logdiag = np.full(dim, np.log(q["sd"]))
    else:
        rng = np.random.default_rng(3)
        if model == "lgcp":
            mean = np.full(dim, np.log(126.0) - 0.955) + 0.05 * rng.standard_normal(dim)
            logdiag = np.full(dim, np.log(q.get("sd", 0.5))) + 0.05 * rng.standard_normal(dim)
        else:
            sig = 15.0 if model == "many_gmm" else 1.0
            mean = 0.3 * rng.standard_normal(dim)
            logdiag = np.log(sig) + 0.1 * rng.standard_normal(dim)
        if "logdiag0" in q:
            logdiag[0] = q["logdiag0"]
    return {"mean": np.asarray(mean, np.float32), "logdiag": np.asarray(logdiag, np.float32)}


@functools.lru_cache(maxsize=None)
def oracle_target_of(model, n_mixes=40):
    if model == "lgcp":
        return otg.Lgcp(lgcp_counts_fixture())
    if model == "many_gmm":
        return otg.ManyGmm(n_mixes=n_mixes)
    return otg.Gmm() if model == "gmm" else otg.Funnel(10)


@functools.lru_cache(maxsize=None)
def device_target_of(model, n_mixes=40):
    from cmcd_amd.lgcp import load_model_lgcp
    from cmcd_amd.model_handler import load_model
    if model == "lgcp":
        return load_model_lgcp("lgcp", None, flat_bin_counts=lgcp_counts_fixture())[0]
    cfg = types.SimpleNamespace(n_mixes=n_mixes) if model == "many_gmm" else types.SimpleNamespace()
    return load_model(model, cfg)[0]


def oracle_side(case):
    """-> (oracle target, dim, float64 vd)."""
    _, model, _, _, extras = case
    return oracle_target_of(model, extras.get("n_mixes", 40)), dim_of(model), {k: v.astype(np.float64) for k, v in q_of(case).items()}


# ------------------------------------------------------------------------------------------ seeds and the floor's guards
@functools.lru_cache(maxsize=None)
def _guards(cid):
    """-> (seeds[n0], near[n0], ridge[n0], floored[n0]) of a floor case from the float64 oracle:
      near   the unfloored log p lies within gated_cases.DELTA (relative) of the floor: float32 and float64 could fall on
             different sides of it;
      ridge  unfloored, below -2000 nats, and the two largest component log-densities within gated_cases.RIDGE_NATS: at such a
             depth a float32 is spaced 1e-4 .. 1e-3, which is the relative error of the mixture weights where two count."""
    case = case_by_id(cid)
    assert is_floor(case) and case[4].get("n_mixes", 40) == 40      # gated_cases.component_gap knows the 40 components
    otarget, dim, vd = oracle_side(case)
    seeds = synthetic.parity_seeds(case[2])
    _, z = orc.mfvi_losses(seeds, vd, dim, otarget)
    lp = otarget.unfloored(z)
    floored = lp <= gc.FLOOR
    near = np.abs(lp - gc.FLOOR) <= gc.DELTA * -gc.FLOOR
    ridge = ~floored & (lp < DEEP) & (gc.component_gap(z) < gc.RIDGE_NATS)
    return seeds, near, ridge, floored


def seeds_of(case):
    """int32 seeds of the case: parity_seeds(n), for a floor case without those the guards drop."""
    if not is_floor(case):
        return synthetic.parity_seeds(case[2])
    seeds, near, ridge, _ = _guards(case[0])
    return np.ascontiguousarray(seeds[~(near | ridge)])


def guard_report(case):
    """-> dict(n0, near, ridge, kept, floored, unfloored): the guards' drop counts and the categories of the survivors."""
    seeds, near, ridge, floored = _guards(case[0])
    keep = ~(near | ridge)
    return dict(n0=len(seeds), near=int(near.sum()), ridge=int((ridge & ~near).sum()), kept=int(keep.sum()),
                floored=int((floored & keep).sum()), unfloored=int((~floored & keep).sum()))


def records_of(case):
    """Records (and gradient rows) the call's reductions see: one per 16-particle tile, on lgcp one per particle."""
    n = len(seeds_of(case))
    return n if case[1] == "lgcp" else (n + 15) // 16


# ------------------------------------------------------------------------------------------ build, reference, gap, bars
def build(case, device="cuda"):
    """-> (target, oracle target, dim, params_flat, unflatten, params_fixed, float64 vd) as test_gpu_mfvi._setup returns them;
    a floor case appends its seeds."""
    from cmcd_amd import boundingmachine as bm
    _, model, _, _, extras = case
    otarget, dim, vd64 = oracle_side(case)
    vdp = {k: torch.from_numpy(v.copy()) for k, v in q_of(case).items()}
    flat, unflatten, fixed = bm.initialize(dim=dim, nbridges=0, vdparams=vdp, trainable=("vd",), device=device)
    out = (device_target_of(model, extras.get("n_mixes", 40)), otarget, dim, flat, unflatten, fixed, vd64)
    return out + (seeds_of(case),) if is_floor(case) else out


def _run(case, dtype):
    otarget, dim, vd = oracle_side(case)
    seeds = seeds_of(case)
    with np.errstate(invalid="ignore", over="ignore"):
        l, z = orc.mfvi_losses(seeds, vd, dim, otarget, dtype=dtype)
        g = orc.mfvi_grad(seeds, vd, dim, otarget, dtype=dtype)
    return np.asarray(l, np.float64), np.asarray(z, np.float64), {k: np.asarray(v, np.float64) for k, v in g.items()}


@functools.lru_cache(maxsize=None)
def _reference(cid):
    return _run(case_by_id(cid), np.float64)


def reference(case):
    """The float64 restatement on the case's seeds, computed once and shared (read-only): (losses, z, {leaf: gradient})."""
    return _reference(case[0])


def leaf_error(a, r):
    """The scale of the leaf-wise gradient comparison: max |a - r| / max(max |r|, 1e-3)."""
    return float(np.abs(np.asarray(a, np.float64) - r).max()) / max(float(np.abs(r).max()), 1e-3)


def worst_particle(l, l_ref):
    """max |l - l_ref| / max(1, |l_ref|) over the finite particles of the reference (0 when there is none)."""
    f = np.isfinite(l_ref)
    return float((np.abs(np.asarray(l, np.float64)[f] - l_ref[f]) / np.maximum(1.0, np.abs(l_ref[f]))).max()) if f.any() else 0.0


@functools.lru_cache(maxsize=None)
def _gap(cid):
    case = case_by_id(cid)
    l64, _, g64 = reference(case)
    l32, _, g32 = _run(case, np.float32)
    assert not np.isnan(l32).any() and np.array_equal(np.isinf(l32), np.isinf(l64)), (cid, "the +inf sets of float32 and float64 differ")
    return worst_particle(l32, l64), {k: leaf_error(g32[k], g64[k]) for k in ("mean", "logdiag")}


def float32_gap(case):
    """The restatement at float32 against float64 on the case's seeds -> (worst-particle relative loss error, {leaf: gradient
    error relative to max(|leaf|, 1e-3)}): what float32 arithmetic alone costs, whatever the kernel."""
    return _gap(case[0])


FLOOR_BAR = 1e-4        # more than 10 x every gap but gmm-narrow-1e-4's; two orders inside the suite's standard 1e-3 / 2e-3


def bar_of(gap):
    """The bar a metric with float32 gap `gap` is held to: max(1e-4, trained_cases.FACTOR x gap)."""
    return max(FLOOR_BAR, tc.FACTOR * gap)


def bars(case):
    """-> (worst-particle bar, {leaf: bar})."""
    gl, gg = float32_gap(case)
    return bar_of(gl), {k: bar_of(v) for k, v in gg.items()}
