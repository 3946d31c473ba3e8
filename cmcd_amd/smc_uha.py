"""Sequential Monte Carlo over the annealing path for 2nd-order CMCD (`MCD_CAIS_UHA_sn`): `cmcd_amd.smc` for a particle state
that carries the momentum.

`segment` is ONE call of libcmcd_hip.so (cmcd_bound_segment_uha, csrc/cmcd_segment_uha.hip): bridges [k0, k1) from q (k0 == 0) or
from the state an earlier segment returned.  A state is a dict of device tensors
    z[N, dim] f32, rho[N, dim] f32, wpath[N] f32, lg[N] f32, key[N, 2] int32 (the uint32 words of gen_k), stats[5] f64, k
where wpath is the path weight WITHOUT the end point's density and lg = log gamma_k(z) + log N(rho; 0, I), so that
-(wpath + lg) is the loss of a chain that stopped at bridge k (at k = K: the loss `bound_forward` returns).  The momentum's
density belongs to lg: the leap-frog is a volume-preserving bijection, so exp(wpath + lg) is a proper weight for
gamma_k(z) N(rho) whatever the network is, and the restart rule of a resampling stage (wpath_j = -lg[a_j]) is the overdamped
one.  Segments compose bit for bit.  `resample_stage` moves z AND rho with the same ancestors — one resampling launch on the rows
[z | rho] — and `smc_bound` drives the whole chain.  Nothing here reads a device value back to the host, so a stage can be
captured into a graph.  The reference has no counterpart; the arithmetic is restated in float64 NumPy in
tests/smc_uha_restatement.py.  No CPU fallback.

LDVI and the UHA boundmode have segments of their own, `cmcd_amd.smc_ldvi` and `cmcd_amd.smc_hais`: they import `resample_stage`
and the driver loop (`_drive`) from here.  Not here: lgcp, the cooperative kernel forms, sharding.  (The reverse-time chain of
this mode: cmcd_amd.reverse_uha.)"""
import ctypes as C

import torch

from . import _lib, resample
from . import mcdboundingmachine as mcdbm
from ._call import consts_args, _inputs, on_device, _workspace
from .smc import _state_tensors, default_cuts, losses_of

__all__ = ["STATE_FIELDS", "segment", "losses_of", "resample_stage", "default_cuts", "smc_bound"]

STATE_FIELDS = ("z", "rho", "wpath", "lg", "key")
MODE = "MCD_CAIS_UHA_sn"


def _state_inputs(state, params_flat, dim, what="a 2nd-order segment", module="smc_uha"):
    """The checks on a state handed to a segment with k0 > 0 -> (z, rho, wpath, key, n)."""
    if not isinstance(state, dict) or any(k not in state for k in ("z", "rho", "wpath", "key")):
        raise TypeError(f"{what} with k0 > 0 starts from the state dict an earlier {module}.segment (or resample_stage) "
                        "returned: z, rho, wpath and key")
    _inputs(None, params_flat, seedless=True)
    return _state_tensors(state, params_flat.device, dim, ("z", "rho", "wpath", "key"))


def segment(state, k0, k1, params_flat, unflatten, params_fixed, log_prob, eps_schedule=None, grad_clipping=False):
    """Bridges [k0, k1) of the 2nd-order forward chain, one library call on the current stream.  `state` is `seeds[N]` at k0 == 0
    (the chain then starts from q exactly as `bound_forward`), otherwise the state of the previous stage, which is left untouched.
    -> the state at bridge k1 (see the module text); its `stats` are the five statistics over -(wpath + lg).
    `MCD_CAIS_UHA_sn` on gmm / funnel / many_gmm only (NotImplementedError otherwise; the overdamped modes: `cmcd_amd.smc`).
    eps_schedule / grad_clipping are accepted for the signature and ignored, as by the forward call of this mode."""
    plan = mcdbm._plan(unflatten, params_fixed, log_prob, eps_schedule, grad_clipping)
    if params_fixed[2] != MODE:
        raise NotImplementedError(f"cmcd_amd.smc_uha runs {MODE} only (boundmode {params_fixed[2]!r}: cmcd_amd.smc)")
    dim, k0, k1 = params_fixed[0], int(k0), int(k1)
    device = params_flat.device
    if k0 == 0:
        seeds, n = _inputs(state, params_flat)
        z = torch.empty((n, dim), dtype=torch.float32, device=device)
        rho = torch.empty((n, dim), dtype=torch.float32, device=device)
        wpath = torch.empty(n, dtype=torch.float32, device=device)
        key = torch.empty((n, 2), dtype=torch.int32, device=device)
    else:
        seeds = None
        z, rho, wpath, key, n = _state_inputs(state, params_flat, dim)

    def launch(dev_index, stream, capturing):
        nbytes = mcdbm._nbytes(plan, "cmcd_segment_uha_workspace_bytes", n)
        ws = _workspace(dev_index, device, stream, capturing, nbytes, "seg_uha",
                        "no 2nd-order segment kernel for this configuration", retire=True)
        cptr, cnum = consts_args(log_prob.consts_on(device))
        lg = torch.empty(n, dtype=torch.float32, device=device)
        stats = torch.empty(_lib.NSTATS, dtype=torch.float64, device=device)
        _lib.check(_lib.lib().cmcd_bound_segment_uha(
            C.byref(plan.desc), C.byref(plan.lay), k0, k1, seeds.data_ptr() if seeds is not None else None, n,
            params_flat.data_ptr(), params_flat.numel(), cptr, cnum,
            ws.data_ptr(), ws.numel(), z.data_ptr(), rho.data_ptr(), wpath.data_ptr(), key.data_ptr(), lg.data_ptr(),
            stats.data_ptr(), stream))
        return {"z": z, "rho": rho, "wpath": wpath, "lg": lg, "key": key, "stats": stats, "k": k1}

    return on_device(device, launch)


def resample_stage(state, groups=1, ess_threshold=0.5, seed=0):
    """`cmcd_amd.smc.resample_stage` for the state with momentum: same trigger, same ln Z column, same restart rule
    (wpath_j = -lg[a_j]); a resampled group takes z AND rho from its ancestors — ONE resampling launch on the rows [z | rho] of
    width 2 dim.  KEYS STAY WITH THEIR SLOT.  Every other group is passed through unchanged (identity ancestors).
    -> (new state, {"resampled"[groups] bool, "ess"[groups], "ln_Z_increment"[groups] f64, "ancestors"[N] int64})."""
    if "rho" not in state:
        raise TypeError("a 2nd-order state carries the momentum: state['rho'] is missing")
    wpath, lg, z, rho = state["wpath"], state["lg"], state["z"], state["rho"]
    n, groups = wpath.numel(), int(groups)
    if groups < 1 or n % groups != 0:
        raise ValueError("N must be a multiple of groups")
    m = n // groups
    dim = z.shape[1]
    zr_res, index, st = resample.resample(losses_of(state), torch.cat([z, rho], dim=1), groups=groups, seed=seed)
    trig = (st["ess"] < float(ess_threshold) * m) & (st["diverged"] == 0) & (st["n_finite"] > 0)
    mask = trig.repeat_interleave(m)
    index = index.to(torch.int64)
    ancestors = torch.where(mask, index, torch.arange(n, dtype=torch.int64, device=wpath.device))
    lg_anc = lg[ancestors]
    new = {k: v for k, v in state.items() if k != "stats"}      # (the statistics described the weights before this stage)
    new["z"] = torch.where(mask[:, None], zr_res[:, :dim], z)
    new["rho"] = torch.where(mask[:, None], zr_res[:, dim:], rho)
    new["wpath"] = torch.where(mask, -lg_anc, wpath)
    new["lg"] = lg_anc
    inc = torch.where(trig, st["ln_Z"], torch.zeros_like(st["ln_Z"]))
    return new, {"resampled": trig, "ess": st["ess"], "ln_Z_increment": inc, "ancestors": ancestors}


def smc_bound(seeds, params_flat, unflatten, params_fixed, log_prob, eps_schedule=None, grad_clipping=False, *, groups=1,
              cuts=None, ess_threshold=0.5, seed=0, trace=False):
    """`cmcd_amd.smc.smc_bound` for `MCD_CAIS_UHA_sn`: the chain of `bound_forward` with resampling stages at the bridges `cuts`.
    Same arguments, same result dict (ln_Z, losses, z, resampled, ess) plus "rho"[N, dim], the final momenta; with trace=True the
    stages carry {"k", "wpath", "lg", "ancestors"} as there.  With ess_threshold = 0 nothing is resampled and losses are the single
    segment [0, K)'s, bit for bit.  Each segment runs the prep launch and evaluates the target at its first state again.  No host
    read."""
    return _drive(segment, seeds, params_flat, unflatten, params_fixed, log_prob, eps_schedule, grad_clipping, groups, cuts,
                  ess_threshold, seed, trace)


def _drive(segment, seeds, params_flat, unflatten, params_fixed, log_prob, eps_schedule, grad_clipping, groups, cuts, ess_threshold,
           seed, trace):
    """The driver loop of `smc_bound` for a state with momentum, with the segment call handed in (this module's, smc_ldvi's,
    smc_hais's): params_fixed[1] is nbridges in all three."""
    K = int(params_fixed[1])
    cuts = default_cuts(K) if cuts is None else [int(c) for c in cuts]
    if any(c <= 0 or c >= K for c in cuts) or any(b <= a for a, b in zip(cuts, cuts[1:])):
        raise ValueError(f"cuts must be ascending bridges inside (0, {K})")
    seeds, n = _inputs(seeds, params_flat)
    groups = int(groups)
    if groups < 1 or n % groups != 0:
        raise ValueError("N must be a multiple of groups")
    args = (params_flat, unflatten, params_fixed, log_prob, eps_schedule, grad_clipping)
    edges = cuts + [K]
    state = segment(seeds, 0, edges[0], *args)
    ln_z = torch.zeros(groups, dtype=torch.float64, device=params_flat.device)
    resampled, ess, stages = [], [], []
    for c, nxt in zip(cuts, edges[1:]):
        arrived = state
        state, info = resample_stage(state, groups, ess_threshold, seed + c)
        ln_z = ln_z + info["ln_Z_increment"]
        resampled.append(info["resampled"])
        ess.append(info["ess"])
        if trace:
            stages.append({"k": c, "wpath": arrived["wpath"], "lg": arrived["lg"], "ancestors": info["ancestors"]})
        state = segment(state, c, nxt, *args)
    losses = losses_of(state)
    final = resample.importance_stats(losses, groups)
    ess.append(final["ess"])
    out = {"ln_Z": ln_z + final["ln_Z"], "losses": losses, "z": state["z"], "rho": state["rho"],
           "resampled": torch.stack(resampled) if resampled else torch.zeros((0, groups), dtype=torch.bool, device=losses.device),
           "ess": torch.stack(ess)}
    if trace:
        stages.append({"k": K, "wpath": state["wpath"], "lg": state["lg"], "ancestors": None})
        out["trace"] = stages
    return out
