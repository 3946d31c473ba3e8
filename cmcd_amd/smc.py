"""Sequential Monte Carlo over the annealing path: the forward chain run in resumable segments, with the particles of a seed
group resampled between bridges when their effective sample size drops.

`segment` is ONE call of libcmcd_hip.so (cmcd_bound_segment, csrc/cmcd_segment.hip): bridges [k0, k1) from q (k0 == 0) or from
the state an earlier segment returned.  A state is a dict of device tensors
    z[N, dim] f32, wpath[N] f32, lg[N] f32, key[N, 2] int32 (the uint32 words of the chain key gen_k), stats[5] f64, k
where wpath is the path weight WITHOUT the end point's density and lg = log gamma_k(z), so that -(wpath + lg) is the loss of a
chain that stopped at bridge k (at k = K: the loss `bound_forward` returns).  Segments compose bit for bit.
`resample_stage` resamples the triggered groups of a state (cmcd_amd.resample, systematic scheme) and `smc_bound` drives the
whole chain.  Nothing here reads a device value back to the host, so a stage can be captured into a graph.  The reference has no
counterpart; the arithmetic is restated in float64 NumPy in tests/smc_restatement.py.  No CPU fallback."""
import ctypes as C

import torch

from . import _lib, resample
from . import mcdboundingmachine as mcdbm
from ._call import consts_args, _inputs, on_device, _workspace

STATE_FIELDS = ("z", "wpath", "lg", "key")


def _state_tensors(state, device, dim, fields):
    """The checks on the tensors of a state handed to a segment with k0 > 0 -> (*fields, n), the fields as fresh tensors the
    library overwrites.  `fields` holds "wpath"[n] and "key"[n, 2]; every other one is a float32 matrix [n, dim]."""
    for name in fields:
        t = state[name]
        if not isinstance(t, torch.Tensor) or t.device != device:
            raise RuntimeError(f"the CMCD hot path runs on a ROCm device only: state[{name!r}] is not a tensor on the device of "
                               "params_flat")
    mats = [f for f in fields if f not in ("wpath", "key")]
    both = lambda names: ", ".join(names[:-1]) + " and " + names[-1] if len(names) > 1 else names[0]
    n = state["wpath"].numel()
    if n < 1 or any(state[f].dtype != torch.float32 for f in mats + ["wpath"]) or state["key"].dtype != torch.int32:
        raise ValueError(f"state: {both(mats + ['wpath'])} must be float32, key int32")
    if any(tuple(state[f].shape) != (n, dim) for f in mats) or tuple(state["key"].shape) != (n, 2):
        raise ValueError(f"state: {both(mats)} must have shape [{n}, {dim}] and key [{n}, 2]")
    fresh = lambda t: t.detach().clone(memory_format=torch.contiguous_format)
    return (*(fresh(state[f].reshape(-1) if f == "wpath" else state[f]) for f in fields), n)


def _state_inputs(state, params_flat, dim):
    """The checks on a state handed to a segment with k0 > 0 -> (z, wpath, key, n)."""
    _inputs(None, params_flat, seedless=True)
    if not isinstance(state, dict) or any(k not in state for k in ("z", "wpath", "key")):
        raise TypeError("a segment with k0 > 0 starts from the state dict an earlier segment (or resample_stage) returned")
    return _state_tensors(state, params_flat.device, dim, ("z", "wpath", "key"))


def segment(state, k0, k1, params_flat, unflatten, params_fixed, log_prob, eps_schedule=None, grad_clipping=False):
    """Bridges [k0, k1) of the forward chain, one library call on the current stream.  `state` is `seeds[N]` at k0 == 0 (the chain
    then starts from q exactly as `bound_forward`), otherwise the state of the previous stage, which is left untouched.
    -> the state at bridge k1 (see the module text); its `stats` are the five statistics over -(wpath + lg).
    Overdamped modes on gmm / funnel / many_gmm only (NotImplementedError otherwise)."""
    plan = mcdbm._plan(unflatten, params_fixed, log_prob, eps_schedule, grad_clipping)
    dim, k0, k1 = params_fixed[0], int(k0), int(k1)
    device = params_flat.device
    if k0 == 0:
        seeds, n = _inputs(state, params_flat)
        z = torch.empty((n, dim), dtype=torch.float32, device=device)
        wpath = torch.empty(n, dtype=torch.float32, device=device)
        key = torch.empty((n, 2), dtype=torch.int32, device=device)
    else:
        seeds = None
        z, wpath, key, n = _state_inputs(state, params_flat, dim)

    def launch(dev_index, stream, capturing):
        what = "no segment kernel for this configuration"
        nbytes = mcdbm._nbytes(plan, "cmcd_segment_workspace_bytes", n)
        if nbytes <= 0 and params_fixed[2] == "MCD_CAIS_UHA_sn":      # the refusal, and where this mode's segments are
            raise NotImplementedError((_lib.last_error() or what)
                                      + " — MCD_CAIS_UHA_sn: cmcd_amd.smc_uha (the state with momentum)")
        ws = _workspace(dev_index, device, stream, capturing, nbytes, "seg", what, retire=True)
        cptr, cnum = consts_args(log_prob.consts_on(device))
        lg = torch.empty(n, dtype=torch.float32, device=device)
        stats = torch.empty(_lib.NSTATS, dtype=torch.float64, device=device)
        _lib.check(_lib.lib().cmcd_bound_segment(
            C.byref(plan.desc), C.byref(plan.lay), k0, k1, seeds.data_ptr() if seeds is not None else None, n,
            params_flat.data_ptr(), params_flat.numel(), cptr, cnum,
            ws.data_ptr(), ws.numel(), z.data_ptr(), wpath.data_ptr(), key.data_ptr(), lg.data_ptr(), stats.data_ptr(),
            stream))
        return {"z": z, "wpath": wpath, "lg": lg, "key": key, "stats": stats, "k": k1}

    return on_device(device, launch)


def losses_of(state):
    """-(wpath + lg): the loss of a chain that stopped at the state's bridge (+inf where lg = -inf: weight 0)."""
    return -(state["wpath"] + state["lg"])


def resample_stage(state, groups=1, ess_threshold=0.5, seed=0):
    """One resampling stage at a cut, per seed group of m = N / groups rows, all on the device (no host read):
    a group is resampled when its ESS < ess_threshold * m, it is not diverged (a NaN or -inf loss) and holds a finite loss.
    A resampled group hands its ln Z column (logsumexp(wpath + lg) - log m) to the running sum, takes z from its ancestors
    (systematic scheme, `resample.resample(..., seed=seed)`) and restarts with uniform weights: wpath_j = -lg[a_j], finite
    because ancestors have positive weight.  KEYS STAY WITH THEIR SLOT: they are not gathered, so two offspring of one ancestor
    draw different noise from here on.  Every other group is passed through unchanged (identity ancestors).
    -> (new state, {"resampled"[groups] bool, "ess"[groups], "ln_Z_increment"[groups] f64, "ancestors"[N] int64})."""
    wpath, lg, z = state["wpath"], state["lg"], state["z"]
    n, groups = wpath.numel(), int(groups)
    if groups < 1 or n % groups != 0:
        raise ValueError("N must be a multiple of groups")
    m = n // groups
    z_res, index, st = resample.resample(losses_of(state), z, groups=groups, seed=seed)
    trig = (st["ess"] < float(ess_threshold) * m) & (st["diverged"] == 0) & (st["n_finite"] > 0)
    mask = trig.repeat_interleave(m)
    index = index.to(torch.int64)
    ancestors = torch.where(mask, index, torch.arange(n, dtype=torch.int64, device=wpath.device))
    lg_anc = lg[ancestors]
    new = {k: v for k, v in state.items() if k != "stats"}      # (the statistics described the weights before this stage)
    new["z"] = torch.where(mask[:, None], z_res.view(z.shape), z)
    new["wpath"] = torch.where(mask, -lg_anc, wpath)
    new["lg"] = lg_anc
    inc = torch.where(trig, st["ln_Z"], torch.zeros_like(st["ln_Z"]))
    return new, {"resampled": trig, "ess": st["ess"], "ln_Z_increment": inc, "ancestors": ancestors}


def default_cuts(nbridges):
    """range(S, K, S) with S = max(1, K // 8): about eight cuts, none at 0 or K."""
    step = max(1, nbridges // 8)
    return list(range(step, nbridges, step))


def smc_bound(seeds, params_flat, unflatten, params_fixed, log_prob, eps_schedule=None, grad_clipping=False, *, groups=1,
              cuts=None, ess_threshold=0.5, seed=0, trace=False):
    """The chain of `bound_forward` with resampling stages at the bridges `cuts` (ascending, inside (0, K); default
    `default_cuts(K)`).  Rows are `groups` consecutive seed groups, each its own particle system; the stage at cut c uses
    `resample_stage(..., seed=seed + c)`.  -> dict of device tensors
        ln_Z[groups] f64     sum of the resampled stages' ln Z columns + logsumexp(wpath + lg) - log m at K
        losses[N] f32        -(wpath + lg) at K: the weights of the final cloud are exp(-losses) within each group
        z[N, dim] f32
        resampled[len(cuts), groups] bool, ess[len(cuts) + 1, groups] f64 (at every cut before resampling, then at K)
    and with trace=True "trace": per stage {"k", "wpath", "lg", "ancestors"} — the state as it ARRIVED at the cut (or at K, where
    ancestors is None).  With ess_threshold = 0 nothing is resampled and losses are the single segment [0, K)'s, bit for bit.
    Each segment runs the prep launch and evaluates its first state again (one extra evaluation per cut).  No host read."""
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
    out = {"ln_Z": ln_z + final["ln_Z"], "losses": losses, "z": state["z"],
           "resampled": torch.stack(resampled) if resampled else torch.zeros((0, groups), dtype=torch.bool, device=losses.device),
           "ess": torch.stack(ess)}
    if trace:
        stages.append({"k": K, "wpath": state["wpath"], "lg": state["lg"], "ancestors": None})
        out["trace"] = stages
    return out
