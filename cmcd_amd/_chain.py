"""What the eight reverse-chain and chain-segment entry points (mcdboundingmachine.bound_reverse, reverse_uha, reverse_ldvi,
reverse_hais; smc, smc_uha, smc_ldvi, smc_hais) do around their own C call, on top of `_call`: the checks on a particle state, the
state's tensors, the cached size query, the outputs, and above one call the resampling stage and the driver loop of `smc_bound`.
A module keeps its gate (which modes it runs, what it says to the others), builds its plan and hands `segment_call` /
`reverse_call` its two C functions, the size query and the call, each with the leading arguments that are the family's own.
Like `_call`, nothing here knows a target or a descriptor; the one place that reads a boundmode is the pair `smc_module` / `reverse_module`, for the two drivers."""
from importlib import import_module

import torch

from . import _lib, resample
from ._call import _inputs, _outputs, _workspace, check_x, consts_args, on_device

_sizes = {}      # (workspace tag, descriptor bytes or shape, n) -> what the call's size query answered: see _ask_size
_SIZE_CACHE = 256


def _ask_size(key, query, qargs, n, what, hint):
    """A size query that `_sizes` does not hold: `query(*qargs, n)`, kept under `key` — a pure function of (query, descriptor or
    shape, n) — when it is > 0.  A refusal (<= 0; the caller raises) is not kept: it is asked again, for its message.  Bounded.
    hint: the module's words behind the library's refusal, raised here."""
    nbytes = query(*qargs, n)
    if nbytes > 0:
        while len(_sizes) >= _SIZE_CACHE:
            _sizes.pop(next(iter(_sizes)))
        _sizes[key] = nbytes
    elif hint:
        raise NotImplementedError((_lib.last_error() or what) + hint)
    return nbytes


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


def _state_inputs(state, params_flat, dim, fields, missing, params_first=False):
    """The checks on a state handed to a segment with k0 > 0 -> (*fields, n).  `missing`: the TypeError text for what is no state
    dict with these fields; params_first: params_flat is checked before the dict (the overdamped call) instead of after it."""
    if params_first:
        _inputs(None, params_flat, seedless=True)
    if not isinstance(state, dict) or any(k not in state for k in fields):
        raise TypeError(missing)
    if not params_first:
        _inputs(None, params_flat, seedless=True)
    return _state_tensors(state, params_flat.device, dim, fields)


def segment_call(state, k0, k1, params_flat, dim, momentum, missing, tag, what, retire, query, qargs, shape, fn, head, consts_on,
                 params_first=False, hint=None):
    """What a `segment` does behind its gate and its plan: bridges [k0, k1) (ints) from `state` = seeds[N] (k0 == 0) or a state dict.
    momentum: the state carries "rho" behind "z"; missing, params_first: see _state_inputs; tag, what, retire: the workspace's
    (`_call._workspace`); query(*qargs, n): the size query, cached under (tag, shape, n) — shape: the descriptor's bytes or what
    stands for it —, hint: see _ask_size; fn(*head, seeds, n, params, n_params, constants, count, workspace, bytes, z, [rho,] wpath,
    key, lg, stats, stream): the C call, whose arguments behind `head` are the same in every family; consts_on(device): the
    target's constants.  -> the state at bridge k1.  (No closure handed in, plain locals, a dict literal: these calls are bound
    by the host at the small shapes, and every Python frame in here is 0.1 .. 0.2 us of them.)"""
    device = params_flat.device
    rho = None
    if k0 == 0:
        seeds, n = _inputs(state, params_flat)
        z = torch.empty((n, dim), dtype=torch.float32, device=device)
        if momentum:
            rho = torch.empty((n, dim), dtype=torch.float32, device=device)
        wpath = torch.empty(n, dtype=torch.float32, device=device)
        key = torch.empty((n, 2), dtype=torch.int32, device=device)
    elif momentum:
        seeds = None
        z, rho, wpath, key, n = _state_inputs(state, params_flat, dim, ("z", "rho", "wpath", "key"), missing, params_first)
    else:
        seeds = None
        z, wpath, key, n = _state_inputs(state, params_flat, dim, ("z", "wpath", "key"), missing, params_first)

    def launch(dev_index, stream, capturing):
        size_key = (tag, shape, n)
        nbytes = _sizes.get(size_key)
        if nbytes is None:
            nbytes = _ask_size(size_key, query, qargs, n, what, hint)
        ws = _workspace(dev_index, device, stream, capturing, nbytes, tag, what, retire=retire)
        cptr, cnum = consts_args(consts_on(device))
        lg = torch.empty(n, dtype=torch.float32, device=device)
        stats = torch.empty(_lib.NSTATS, dtype=torch.float64, device=device)
        sptr = seeds.data_ptr() if seeds is not None else None
        if momentum:
            _lib.check(fn(*head, sptr, n, params_flat.data_ptr(), params_flat.numel(), cptr, cnum, ws.data_ptr(), ws.numel(),
                          z.data_ptr(), rho.data_ptr(), wpath.data_ptr(), key.data_ptr(), lg.data_ptr(), stats.data_ptr(), stream))
            return {"z": z, "rho": rho, "wpath": wpath, "lg": lg, "key": key, "stats": stats, "k": k1}
        _lib.check(fn(*head, sptr, n, params_flat.data_ptr(), params_flat.numel(), cptr, cnum, ws.data_ptr(), ws.numel(),
                      z.data_ptr(), wpath.data_ptr(), key.data_ptr(), lg.data_ptr(), stats.data_ptr(), stream))
        return {"z": z, "wpath": wpath, "lg": lg, "key": key, "stats": stats, "k": k1}

    return on_device(device, launch)


def reverse_call(seeds, x, params_flat, dim, momentum, tag, what, retire, query, qargs, shape, fn, head, consts_on):
    """What a `bound_reverse` does behind its gate and its plan.  momentum: the chain returns its end momentum rho0; the other
    arguments as for segment_call, with fn(*head, seeds, x, n, params, n_params, constants, count, workspace, bytes, w, z0, [rho0,]
    stats, stream); a callable `head` is resolved right in front of the C call.  -> (w, z0, [rho0,] stats)."""
    seeds, n = _inputs(seeds, params_flat)
    device = params_flat.device
    check_x(x, n, dim, device)

    def launch(dev_index, stream, capturing):
        size_key = (tag, shape, n)
        nbytes = _sizes.get(size_key)
        if nbytes is None:
            nbytes = _ask_size(size_key, query, qargs, n, what, None)
        ws = _workspace(dev_index, device, stream, capturing, nbytes, tag, what, retire=retire)
        cptr, cnum = consts_args(consts_on(device))
        w, z0, stats = _outputs(n, dim, device)
        rho0 = torch.empty((n, dim), dtype=torch.float32, device=device) if momentum else None
        h = head() if callable(head) else head
        if momentum:
            _lib.check(fn(*h, seeds.data_ptr(), x.data_ptr(), n, params_flat.data_ptr(), params_flat.numel(), cptr, cnum,
                          ws.data_ptr(), ws.numel(), w.data_ptr(), z0.data_ptr(), rho0.data_ptr(), stats.data_ptr(), stream))
            return w, z0, rho0, stats
        _lib.check(fn(*h, seeds.data_ptr(), x.data_ptr(), n, params_flat.data_ptr(), params_flat.numel(), cptr, cnum,
                      ws.data_ptr(), ws.numel(), w.data_ptr(), z0.data_ptr(), stats.data_ptr(), stream))
        return w, z0, stats

    return on_device(device, launch)


def eubo_of(out):
    """-> (EUBO = mean(w), (w, z0)) of what a `bound_reverse` of this package returned, (w, z0, [rho0,] stats): the one body
    of every module's `compute_reverse_bound`."""
    w, z0, stats = out[0], out[1], out[-1]
    return (stats[1] / w.numel()).to(torch.float32), (w, z0)


def losses_of(state):
    """-(wpath + lg): the loss of a chain that stopped at the state's bridge (+inf where lg = -inf: weight 0)."""
    return -(state["wpath"] + state["lg"])


def resample_stage(state, groups=1, ess_threshold=0.5, seed=0, momentum=False):
    """One resampling stage at a cut (`smc.resample_stage` has the rule).  momentum: the state carries rho, which moves with z —
    ONE resampling launch on the rows [z | rho]; otherwise z goes to the launch as it is."""
    if momentum and "rho" not in state:
        raise TypeError("a 2nd-order state carries the momentum: state['rho'] is missing")
    wpath, lg, z = state["wpath"], state["lg"], state["z"]
    n, groups = wpath.numel(), int(groups)
    if groups < 1 or n % groups != 0:
        raise ValueError("N must be a multiple of groups")
    m = n // groups
    rows = torch.cat([z, state["rho"]], dim=1) if momentum else z
    res, index, st = resample.resample(losses_of(state), rows, groups=groups, seed=seed)
    trig = (st["ess"] < float(ess_threshold) * m) & (st["diverged"] == 0) & (st["n_finite"] > 0)
    mask = trig.repeat_interleave(m)
    index = index.to(torch.int64)
    ancestors = torch.where(mask, index, torch.arange(n, dtype=torch.int64, device=wpath.device))
    lg_anc = lg[ancestors]
    new = {k: v for k, v in state.items() if k != "stats"}      # (the statistics described the weights before this stage)
    if momentum:
        dim = z.shape[1]
        new["z"] = torch.where(mask[:, None], res[:, :dim], z)
        new["rho"] = torch.where(mask[:, None], res[:, dim:], state["rho"])
    else:
        new["z"] = torch.where(mask[:, None], res.view(z.shape), z)
    new["wpath"] = torch.where(mask, -lg_anc, wpath)
    new["lg"] = lg_anc
    inc = torch.where(trig, st["ln_Z"], torch.zeros_like(st["ln_Z"]))
    return new, {"resampled": trig, "ess": st["ess"], "ln_Z_increment": inc, "ancestors": ancestors}


def default_cuts(nbridges):
    """range(S, K, S) with S = max(1, K // 8): about eight cuts, none at 0 or K."""
    step = max(1, nbridges // 8)
    return list(range(step, nbridges, step))


def drive(segment, momentum, seeds, params_flat, unflatten, params_fixed, log_prob, eps_schedule, grad_clipping, groups, cuts,
          ess_threshold, seed, trace):
    """The driver loop of every `smc_bound`, with the module's segment call handed in (`smc.smc_bound` has the result dict;
    momentum: it also holds "rho", the final momenta).  params_fixed[1] is nbridges in all four families.  The stages are this
    module's `resample_stage`, not the name a module re-exports: replacing `smc.resample_stage` does not reach `smc.smc_bound`."""
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
        state, info = resample_stage(state, groups, ess_threshold, seed + c, momentum)
        ln_z = ln_z + info["ln_Z_increment"]
        resampled.append(info["resampled"])
        ess.append(info["ess"])
        if trace:
            stages.append({"k": c, "wpath": arrived["wpath"], "lg": arrived["lg"], "ancestors": info["ancestors"]})
        state = segment(state, c, nxt, *args)
    losses = losses_of(state)
    final = resample.importance_stats(losses, groups)
    ess.append(final["ess"])
    out = {"ln_Z": ln_z + final["ln_Z"], "losses": losses, "z": state["z"], **({"rho": state["rho"]} if momentum else {}),
           "resampled": torch.stack(resampled) if resampled else torch.zeros((0, groups), dtype=torch.bool, device=losses.device),
           "ess": torch.stack(ess)}
    if trace:
        stages.append({"k": K, "wpath": state["wpath"], "lg": state["lg"], "ancestors": None})
        out["trace"] = stages
    return out


_FAMILY = {"MCD_CAIS_UHA_sn": "uha", "MCD_U_a-lp-sn": "ldvi", "MCD_U_a-lp": "ldvi", "UHA": "hais"}


def smc_module(boundmode):
    """The module whose `segment` / `smc_bound` run `boundmode`: smc_uha, smc_ldvi, smc_hais, or smc for every other mode."""
    return import_module(".smc" + ("_" + _FAMILY[boundmode] if boundmode in _FAMILY else ""), __package__)


def reverse_module(boundmode):
    """The module whose `bound_reverse` runs `boundmode`: reverse_uha, reverse_ldvi, reverse_hais, or mcdboundingmachine."""
    return import_module(".reverse_" + _FAMILY[boundmode] if boundmode in _FAMILY else ".mcdboundingmachine", __package__)
