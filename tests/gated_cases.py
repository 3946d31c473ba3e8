"""Gradient cases in which the three hard gates of the training gradients ACT, shared by tests/test_oracle_grad.py (which
asserts on the CPU, on the float64 oracle, that each case does what it is here for) and the GPU gradient tests.

The gates (each makes a derivative exactly zero):
  floor  many_gmm sets log p = -inf where the mixture's log-density is <= -1e4; score and Hessian are zero there;
  clip   grad_clipping clips grad log p to +-1e3 (MCD_CAIS_sn), grad log p and grad log q to +-1e2 (MCD_CAIS_var_sn); the
         2nd-order mode always clips grad log p to +-1e2; a clipped coordinate passes no derivative;
  clamp  the dds net clamps its output to +-1e4; a clamped output passes nothing back into the net.

A case is `(id, config, overrides, seeds, mode)`.  `overrides` go to cmcd_amd.synthetic.build, except the keys of EDITS, which
`build_case` applies to the built parameters.  `seeds` are the survivors of `synthetic.parity_seeds(n0)`, n0 = the last seed:
particles whose own chain comes within DELTA of a threshold (under either parameter set) are dropped, so that the float32
kernels and the float64 oracle cannot fall on different sides of a gate (tests/test_oracle_grad.py re-derives the list).
"""
import numpy as np
import torch

from cmcd_amd import synthetic
from oracle import cmcd_oracle as orc
from oracle import cmcd_oracle_torch as ot

FLOOR = -1e4
CLAMP = 1e4
CLIP = {"MCD_CAIS_sn": 1e3, "MCD_CAIS_var_sn": 1e2, "MCD_CAIS_UHA_sn": 1e2}

# Relative guard band around every threshold.  Measured (`float32_gap`: the NumPy oracle in float32 against float64 on the
# cases' own seeds, worst |x32 - x64| / max(|x64|, threshold) over every traced quantity, case and parameter set):
# 3.9e-5 (uha-floor, sparse set: float32 positions of order 160 under a score of order 200; every other case is below
# 1.5e-5).  The band is ten times that; tests/test_oracle_grad.py re-measures the gap and holds it to DELTA / 10.
MEASURED_GAP = 3.9e-5
DELTA = 4e-4

# leaf-wise bar of the GPU comparison (test_gpu_grad._compare); a gate counts as tested when opening it moves one leaf or
# more by over ten times that
BAR = 2e-3
SEPARATION = 10 * BAR

EDITS = ("out_scale", "out_shift", "logdiag_add", "mean_add")

_S17 = tuple(range(1, 18))
_S33 = tuple(range(1, 34))
_MANY = "many_gmm_n2000_k256_dds"

GATED_CASES = [
    # q sits beyond the floor (mean x = 180, modes within +-40) and the net's output bias carries the particles inwards:
    # floored at the first evaluations, inside at z_K
    ("floor-mid", _MANY, dict(nbridges=4, init_sigma=40.0, mean_add=(180.0, 0.0), out_shift=(40.0, 0.0)), _S33, "MCD_CAIS_sn"),
    # sigma 60 floors 2 % of a batch, too few for 17 particles: sigma 150
    ("floor-end", _MANY, dict(nbridges=4, init_sigma=150.0), _S17, "MCD_CAIS_sn"),
    ("clip-p-1e3", "gmm_n300_k8", dict(nbridges=4, grad_clipping=True, init_sigma=200.0),
     tuple(s for s in range(1, 35) if s != 14), "MCD_CAIS_sn"),
    # q: x around 110 (55 to 105 units right of the nearest mode), y with std 0.05 (grad log q = 400 dy)
    ("clip-pq-1e2", "many_gmm_var_n16000_k256", dict(nbridges=4, init_eps=0.05, init_sigma=15.0, mean_add=(110.0, 0.0),
                                                     logdiag_add=(0.0, -5.7)), _S33, "MCD_CAIS_var_sn"),
    # eps 0.01: at the configuration's 0.1 one clipped step of 33 units carries v out of the clipped region
    ("clip-funnel", "funnel_n300_k64", dict(nbridges=2, grad_clipping=True, init_sigma=15.0, init_eps=0.01), _S17, "MCD_CAIS_sn"),
    ("clamp-dds-gmm", "gmm_n300_k8", dict(nbridges=2, nn_arch="dds", init_eps=1e-3, out_scale=1e5, out_shift=(9e3, -9e3)),
     tuple(s for s in range(1, 19) if s != 8), "MCD_CAIS_sn"),
    ("clamp-dds-funnel", "funnel_n300_k64", dict(nbridges=2, nn_arch="dds", init_eps=1e-4, out_scale=1e6), _S17, "MCD_CAIS_sn"),
    ("uha-floor", _MANY, dict(nbridges=4, init_eps=1.0, init_gamma=1.0, init_sigma=30.0, mean_add=(160.0, 0.0),
                              out_shift=(20.0, 0.0)), _S33, "MCD_CAIS_UHA_sn"),
    ("uha-clamp", "gmm_n300_k8", dict(nbridges=2, nn_arch="dds", init_gamma=3.0, init_eps=1e-3, out_scale=1e5,
                                      out_shift=(9e3, -9e3)), _S17, "MCD_CAIS_UHA_sn"),
    # no network in this mode's forward kernel, so nothing carries a floored particle back: floored evaluations are counted
    ("ula_sn-floor", _MANY, dict(nbridges=4, init_eps=0.05, init_sigma=150.0), _S17, "MCD_ULA_sn"),
]

# case id -> the gate the case is here for
GATE = {"floor-mid": "floor", "floor-end": "floor", "clip-p-1e3": "clip", "clip-pq-1e2": "clip", "clip-funnel": "clip",
        "clamp-dds-gmm": "clamp", "clamp-dds-funnel": "clamp", "uha-floor": "floor", "uha-clamp": "clamp",
        "ula_sn-floor": "floor"}
# case id -> which share `gate_share` measures (see there)
CONDITION = {"floor-mid": "floor-mid", "floor-end": "floor-end", "clip-p-1e3": "clip", "clip-pq-1e2": "clip",
             "clip-funnel": "clip-funnel", "clamp-dds-gmm": "clamp", "clamp-dds-funnel": "clamp", "uha-floor": "floor-mid",
             "uha-clamp": "clamp", "ula_sn-floor": "floor-evals"}


def case_by_id(cid):
    return next(c for c in GATED_CASES if c[0] == cid)


def cases_of(*modes):
    return [c for c in GATED_CASES if c[4] in modes]


def build_case(case, device="cpu"):
    """synthetic.build for the case, with its parameter edits: out_scale multiplies the dds output layer's weights, out_shift
    is added to its bias, logdiag_add / mean_add to log std / mean of q (per dimension)."""
    cid, config, over, seeds, mode = case
    over = dict(over)
    edits = {k: over.pop(k) for k in EDITS if k in over}
    b = synthetic.build(config, device="cpu", boundmode=mode, **over)
    flat = b["params_flat"].clone()
    train, notrain = b["unflatten"](flat)     # views of `flat`
    allp = {**train, **notrain}
    if "out_scale" in edits:
        allp["sn"]["drift_net/~/linear_zero"]["w"].mul_(float(edits["out_scale"]))
    if "out_shift" in edits:
        allp["sn"]["drift_net/~/linear_zero"]["b"].add_(torch.tensor(edits["out_shift"], dtype=torch.float32))
    if "logdiag_add" in edits:
        allp["vd"]["logdiag"].add_(torch.tensor(edits["logdiag_add"], dtype=torch.float32))
    if "mean_add" in edits:
        allp["vd"]["mean"].add_(torch.tensor(edits["mean_add"], dtype=torch.float32))
    b["params_flat"] = flat.to(device)
    return b


def oracle(b, seeds, straight_through=None, trace=None):
    """-> (value, losses, z, grads) of the float64 autograd oracle on the built case."""
    cfg = b["cfg"]
    dim, K, mode, spec = b["params_fixed"]
    p = synthetic.oracle_params(b["unflatten"], b["params_flat"])
    return ot.bound_and_grad(np.asarray(seeds, np.int32), p, dim, K, mode, spec.arch, cfg["model"], cfg["eps_schedule"],
                             cfg["grad_clipping"], trace=trace, straight_through=straight_through)


def thresholds(b):
    """{trace key: threshold} of the gates that exist in this configuration."""
    cfg = b["cfg"]
    _, _, mode, spec = b["params_fixed"]
    th = {}
    if cfg["model"] == "many_gmm":
        th["lp"] = -FLOOR
    if mode == "MCD_CAIS_UHA_sn":
        th["gp"] = CLIP[mode]
    elif cfg["grad_clipping"] and mode in CLIP:
        th["gp"] = CLIP[mode]
        if mode == "MCD_CAIS_var_sn":
            th["gq"] = CLIP[mode]
    if spec.arch == "dds" and mode != "MCD_ULA":
        th["out"] = CLAMP
    return th


def _stack(trace, key):
    a = np.stack(trace[key])                      # [evaluations, N] or [evaluations, N, dim]
    return a if a.ndim == 3 else a[:, :, None]


def band_violations(b, trace):
    """bool [N]: the particle has a traced value within DELTA (relative) of a threshold it is compared with."""
    bad = None
    for key, thr in thresholds(b).items():
        a = np.abs(_stack(trace, key))
        near = (np.abs(a - thr) <= DELTA * thr).any(axis=(0, 2))
        bad = near if bad is None else bad | near
    return bad


def band_margin(b, trace):
    """Smallest relative distance of any traced value to its threshold."""
    return min(float((np.abs(np.abs(_stack(trace, key)) - thr) / thr).min()) for key, thr in thresholds(b).items())


def gate_share(case, b, trace):
    """{name: share in [0, 1]} of the evaluations at which the case's gate acts; every entry must lie in [0.1, 0.9].
      floor-mid   particles floored at an intermediate evaluation and not at z_K;
      floor-end   particles floored at z_K;
      floor-evals (particle, evaluation) pairs floored;
      clip        (particle, evaluation, coordinate) with |grad log p| beyond the clip ("gp"), the same for grad log q where it
                  is clipped ("gq"); "funnel": additionally the first coordinate and the others, each on their own;
      clamp       (particle, network call, coordinate) with the pre-clamp output beyond +-1e4."""
    cid = case[0]
    th = thresholds(b)
    cond = CONDITION[cid]
    if cond in ("floor-mid", "floor-end", "floor-evals"):
        fl = _stack(trace, "lp")[:, :, 0] <= FLOOR            # [evaluations, N]; the last one is z_K
        if cond == "floor-evals":
            return {"floored evaluations": float(fl.mean())}
        if cond == "floor-end":
            return {"floored at z_K": float(fl[-1].mean())}
        return {"floored mid-chain only": float((fl[:-1].any(0) & ~fl[-1]).mean())}
    if cond.startswith("clip"):
        gp = np.abs(_stack(trace, "gp")) > th["gp"]
        out = {"gp": float(gp.mean())}
        if "gq" in th:
            out["gq"] = float((np.abs(_stack(trace, "gq")) > th["gq"]).mean())
        if cond == "clip-funnel":
            out = {"gp[0]": float(gp[:, :, 0].mean()), "gp[1:]": float(gp[:, :, 1:].mean())}
        return out
    assert cond == "clamp"
    return {"out": float((np.abs(_stack(trace, "out")) > CLAMP).mean())}


def select_seeds(case, n0):
    """The survivors of parity_seeds(n0): particles whose chain violates the guard band under either parameter set are dropped
    (each particle's chain is its own: dropping one does not change another)."""
    seeds = synthetic.parity_seeds(n0)
    bad = np.zeros(n0, bool)
    saved = synthetic.DENSE_DEFAULT
    try:
        for dense in (False, True):
            synthetic.DENSE_DEFAULT = dense
            b = build_case(case)
            trace = {}
            oracle(b, seeds, trace=trace)
            bad |= band_violations(b, trace)
    finally:
        synthetic.DENSE_DEFAULT = saved
    return tuple(int(s) for s in seeds[~bad])


def float32_gap(case, b):
    """Worst |x32 - x64| / max(|x64|, threshold) over the traced quantities of the NumPy oracle run in float32 and float64."""
    from helpers import oracle_target
    cfg = b["cfg"]
    dim, K, mode, spec = b["params_fixed"]
    p = synthetic.oracle_params(b["unflatten"], b["params_flat"])
    tr = {}
    for dt in (np.float32, np.float64):
        tr[dt] = {}
        orc.compute_log_elbo_batch(np.asarray(case[3], np.int32), p, dim, K, mode, spec.arch, oracle_target(cfg),
                                   eps_schedule=cfg["eps_schedule"], grad_clipping=cfg["grad_clipping"], dtype=dt,
                                   trace=tr[dt])
    worst = 0.0
    for key, thr in thresholds(b).items():
        a32, a64 = _stack(tr[np.float32], key).astype(np.float64), _stack(tr[np.float64], key)
        worst = max(worst, float((np.abs(a32 - a64) / np.maximum(np.abs(a64), thr)).max()))
    return worst


def leaf_separation(g_true, g_open):
    """{leaf path: max |open - true| / max |true|} over the oracle's gradient dicts."""
    out = {}

    def walk(a, c, path):
        for k in a:
            if isinstance(a[k], dict):
                walk(a[k], c[k], path + (k,))
            else:
                scale = float(np.abs(a[k]).max())
                diff = float(np.abs(np.asarray(c[k]) - np.asarray(a[k])).max())
                out["/".join(path + (k,))] = diff / scale if scale > 0 else (np.inf if diff > 0 else 0.0)
    walk(g_true, g_open, ())
    return out


# ------------------------------------------------------------------------------------------ UHA (cmcd_amd.hais)
# The plain Hamiltonian AIS mode has no network, clip or clamp: its one gate is the many_gmm floor, which the forward kernel
# meets in Target::eval and the reverse sweep in Target::eval_hess.  The yardstick is tests/hais_restatement.py.
#
# q = N((150, 0), ~15^2) sits beyond the floor (modes within +-40; log p <= -1e4 from about 105 units off the nearest mode)
# and eps = 1: a floored particle feels grad log q alone and drifts on its momentum; one that comes inside is kicked by a
# score of order 190 and may shoot through the modes and out on the far side.  Of the seeds 1 .. 2048 some therefore come
# inside before z_K, a few cross outwards and end floored, most stay floored and a quarter never are.
#
# Two guards decide which seeds may be used, both from the float64 restatement alone:
#   band   an evaluation within DELTA (relative) of the floor: float32 and float64 could fall on different sides.  8 seeds.
#   ridge  an unfloored evaluation at which the two largest component log-densities are within RIDGE_NATS = 16 nats.  At a
#          log-density of order -1e4 a float32 is spaced 1e-3, so the mixture weights (a softmax of such numbers) carry a
#          relative error of 1e-3 wherever two components both count; with eps = 1 and a Hessian of order (d / s^2)^2 / 4 ~ 80
#          across the ridge between two modes d ~ 10 apart, the chain amplifies it.  Measured per particle on the first 120
#          unfloored seeds: float32 restatement against float64, worst leaf, as a share of the batch gradient: up to 2.5e-2
#          where the gap is below 8 nats, below 1.3e-5 above 8 nats, below 1.2e-6 above 16 nats.  e^-16 = 1.1e-7 is a float32's
#          unit roundoff: beyond it the second component does not reach the sum.  Without this guard the batch's gap was
#          7.7e-3 (vd/logdiag), with smaller eps or a nearer q anything between 1e-7 and 0.5, by which seeds hit a ridge.
# Categories of the band-clear seeds: 118 floored at early evaluations and inside at z_K, 6 that end floored after an
# unfloored evaluation, 1361 floored at every evaluation, 555 never floored.  The batch takes the first 16 / 4 / 5 / 8 of
# them that are clear of the ridge guard too, in seed order.  tests/test_hais_oracle.py re-derives every figure.
HAIS_FLOOR = dict(target="many_gmm", dim=2, K=4, L=2, eps=1.0, eta=0.6, seed=3, sigma=15.0, mean_scale=0.0,
                  mean_add=(150.0, 0.0), pool=2048, take=(16, 4, 5, 8))
HAIS_FLOOR_CATEGORIES = ("floored mid-chain, inside at z_K", "ends floored", "floored throughout", "never floored")
RIDGE_NATS = 16.0


def hais_floor_params(device="cpu"):
    import hais_restatement as hr
    c = HAIS_FLOOR
    return hr.make_params(c["dim"], c["K"], c["L"], c["eps"], eta=c["eta"], seed=c["seed"], sigma=c["sigma"],
                          mean_scale=c["mean_scale"], mean_add=c["mean_add"], device=device)


def component_gap(z):
    """[..., 2] positions -> the two largest component log-densities of many_gmm apart, in nats (float64)."""
    import math
    from oracle.targets import many_gmm_means
    mu = np.asarray(many_gmm_means(40, 2, 40.0), np.float64)
    s = math.log1p(math.exp(0.1))
    comp = -0.5 * (((np.asarray(z, np.float64)[..., None, :] - mu) / s) ** 2).sum(-1)
    top = np.sort(comp, axis=-1)[..., -2:]
    return top[..., 1] - top[..., 0]


_hais_floor_cache = {}


def hais_floor_pool():
    """-> (seeds[pool], near[pool] bool: an evaluation within DELTA of the floor, ridge[pool] bool: an unfloored evaluation
    within RIDGE_NATS of a ridge, category[pool] in 0 .. 3 (the index into HAIS_FLOOR_CATEGORIES)), from the unfloored log p
    and the positions of the float64 restatement at every one of the K L + 1 evaluations."""
    if "pool" not in _hais_floor_cache:
        import hais_restatement as hr
        c = HAIS_FLOOR
        flat, un, fixed = hais_floor_params()
        seeds = np.arange(1, c["pool"] + 1, dtype=np.int32)
        trace = {}
        hr.forward(seeds, hr.params_numpy(un, flat), c["dim"], c["K"], c["L"], c["target"], trace=trace)
        lp = np.stack(trace["lp"])                             # [K L + 1, pool]
        assert lp.shape == (c["K"] * c["L"] + 1, c["pool"])
        near = (np.abs(lp - FLOOR) <= DELTA * -FLOOR).any(0)
        fl = lp <= FLOOR
        ridge = ((component_gap(np.stack(trace["z"])) < RIDGE_NATS) & ~fl).any(0)
        cat = np.where(fl.all(0), 2, np.where(fl[-1], 1, np.where(fl.any(0), 0, 3)))
        _hais_floor_cache["pool"] = (seeds, near, ridge, cat)
    return _hais_floor_cache["pool"]


def hais_floor_batch():
    """-> (seeds[33] in seed order, category[33]): the first take[k] seeds of every category that both guards leave."""
    seeds, near, ridge, cat = hais_floor_pool()
    ok = ~near & ~ridge
    pick = np.sort(np.concatenate([np.flatnonzero(ok & (cat == k))[:t] for k, t in enumerate(HAIS_FLOOR["take"])]))
    return seeds[pick], cat[pick]
