"""Sequential Monte Carlo over the annealing path for UHA (Hamiltonian AIS, `config.boundmode = "UHA"`): `cmcd_amd.smc_uha` for
the second of the two momentum baselines.

`segment` is ONE call of libcmcd_hip.so (cmcd_bound_segment_hais, csrc/cmcd_segment_hais.hip): bridges [k0, k1) of the chain of
`hais.bound_forward` from q (k0 == 0) or from the state an earlier segment returned.  A state is smc_uha's dict of device tensors
    z[N, dim] f32, rho[N, dim] f32, wpath[N] f32, lg[N] f32, key[N, 2] int32 (the uint32 words of gen_k), stats[5] f64, k
where rho is the momentum BETWEEN bridges (what the next refresh starts from; exp(md) normal(R) at k = 0) and lg = log gamma_k(z)
ALONE: the refresh is reversible with respect to N(0, exp(md)^2), so the momentum densities of the forward functional telescope
and it has neither an initial nor a final momentum term (the derivation is written out in include/cmcd_hip.h).  -(wpath + lg) is
the loss of a chain that stopped at bridge k (at k = K: the loss `hais.bound_forward` returns), exp(wpath + lg) a proper weight
for gamma_k(z) N(rho; 0, exp(md)^2) on the pair (z, rho) — so the restart rule of a resampling stage is the overdamped one and
a stage must move rho with z.  Segments compose bit for bit; a cut costs one extra target evaluation.  `resample_stage` is
smc_uha's as it stands (one resampling launch on the rows [z | rho], keys stay with their slot) and `smc_bound` runs smc_uha's
driver loop on this module's segment call.  Nothing here reads a device value back to the host, so a stage can be captured into
a graph.  The reference has no counterpart; the arithmetic is restated in float64 NumPy in tests/smc_hais_restatement.py.  No CPU
fallback.

Not here: lgcp (`cmcd_amd.hais_lgcp` runs whole chains only), a cooperative kernel form, sharding of segments."""
from . import _chain, _lib
from . import hais
from ._chain import default_cuts, losses_of
from .smc_uha import STATE_FIELDS, _missing, resample_stage

__all__ = ["STATE_FIELDS", "segment", "losses_of", "resample_stage", "default_cuts", "smc_bound"]

_MISSING = _missing("a UHA segment", "smc_hais")


def _fixed(params_fixed, log_prob):
    """`hais.initialize`'s params_fixed = (dim, nbridges, lfsteps), checked in the order of `reverse_hais.bound_reverse`."""
    if len(params_fixed) != 3:      # (dim, nbridges, mode, apply_fun_sn): an MCD mode
        mode = params_fixed[2] if len(params_fixed) == 4 else None
        where = ("cmcd_amd.smc_uha" if mode == "MCD_CAIS_UHA_sn" else
                 "cmcd_amd.smc_ldvi" if mode in ("MCD_U_a-lp-sn", "MCD_U_a-lp") else "cmcd_amd.smc")
        raise NotImplementedError(f"cmcd_amd.smc_hais runs the UHA boundmode only (this params_fixed: {where})")
    dim, nbridges, lfsteps = params_fixed
    if not hasattr(log_prob, "target_id"):
        raise TypeError("log_prob must be a cmcd_amd.model_handler.Target (see load_model)")
    if log_prob.dim != dim:
        raise ValueError(f"target dim {log_prob.dim} != params_fixed dim {dim}")
    if nbridges < 1 or lfsteps < 1:
        raise ValueError(f"nbridges = {nbridges}, lfsteps = {lfsteps}: chain segments need nbridges >= 1 and lfsteps >= 1")
    return dim, nbridges, lfsteps


def segment(state, k0, k1, params_flat, unflatten, params_fixed, log_prob, eps_schedule=None, grad_clipping=False):
    """Bridges [k0, k1) of the UHA forward chain, one library call on the current stream; `params_fixed` is `hais.initialize`'s
    (dim, nbridges, lfsteps).  `state` is `seeds[N]` at k0 == 0 (the chain then starts from q exactly as `hais.bound_forward`),
    otherwise the state of the previous stage, which is left untouched.  -> the state at bridge k1 (see the module text); its
    `stats` are the five statistics over -(wpath + lg).  gmm / funnel / many_gmm only (NotImplementedError otherwise, lgcp
    included; the MCD modes: `cmcd_amd.smc`, `cmcd_amd.smc_uha`, `cmcd_amd.smc_ldvi`).  eps_schedule / grad_clipping are
    accepted for the signature and ignored: the mode has neither."""
    shape = _fixed(params_fixed, log_prob)
    k0, k1 = int(k0), int(k1)
    L, shape = _lib.lib(), (log_prob.target_id, *shape)
    # the offsets of an Unflatten never change: hais._layout builds the struct once per tree.  (No prep tables in this mode:
    # nothing to retire)
    return _chain.segment_call(
        state, k0, k1, params_flat, shape[1], True, _MISSING, "seg_hais", "no Hamiltonian AIS segment kernel for this target",
        False, L.cmcd_segment_hais_workspace_bytes, shape, shape,
        L.cmcd_bound_segment_hais, (*shape, hais._layout(unflatten), k0, k1), log_prob.consts_on)


def smc_bound(seeds, params_flat, unflatten, params_fixed, log_prob, eps_schedule=None, grad_clipping=False, *, groups=1,
              cuts=None, ess_threshold=0.5, seed=0, trace=False):
    """`cmcd_amd.smc_uha.smc_bound` for UHA: the chain of `hais.bound_forward` with resampling stages at the bridges `cuts`.
    Same arguments, same result dict (ln_Z, losses, z, rho, resampled, ess; with trace=True the stages); "rho" holds the momenta
    that left the last bridge.  With ess_threshold = 0 nothing is resampled and losses are the single segment [0, K)'s, bit for
    bit.  No host read."""
    _fixed(params_fixed, log_prob)
    return _chain.drive(segment, True, seeds, params_flat, unflatten, params_fixed, log_prob, eps_schedule, grad_clipping, groups,
                        cuts, ess_threshold, seed, trace)
