"""Sequential Monte Carlo over the annealing path for LDVI (`MCD_U_a-lp-sn` and its network-free sibling `MCD_U_a-lp`):
`cmcd_amd.smc_uha` for the first of the two momentum baselines.

`segment` is ONE call of libcmcd_hip.so (cmcd_bound_segment_ldvi, csrc/cmcd_segment_ldvi.hip): bridges [k0, k1) of the chain of
`ldvi.bound_forward` from q (k0 == 0) or from the state an earlier segment returned.  A state is smc_uha's dict of device tensors
    z[N, dim] f32, rho[N, dim] f32, wpath[N] f32, lg[N] f32, key[N, 2] int32 (the uint32 words of gen_k), stats[5] f64, k
with lg = log gamma_k(z) + log N(rho; 0, I), so that -(wpath + lg) is the loss of a chain that stopped at bridge k (at k = K: the
loss `ldvi.bound_forward` returns).  The leap-frog is a volume-preserving bijection of (z, rho), so exp(wpath + lg) is a proper
weight for gamma_k(z) N(rho) and the restart rule of a resampling stage is the overdamped one.  Segments compose bit for bit.
`resample_stage` is smc_uha's as it stands (one resampling launch on the rows [z | rho], keys stay with their slot) and
`smc_bound` runs smc_uha's driver loop on this module's segment call.  Nothing here reads a device value back to the host, so a
stage can be captured into a graph.  The reference has no counterpart; the arithmetic is written out in include/cmcd_hip.h and
restated in float64 NumPy in tests/smc_ldvi_restatement.py.  No CPU fallback.

Not here: lgcp, a cooperative kernel form, sharding of segments."""
import ctypes as C

from . import _chain, _lib
from . import ldvi
from ._chain import default_cuts, losses_of
from .smc_uha import STATE_FIELDS, _missing, resample_stage

__all__ = ["STATE_FIELDS", "segment", "losses_of", "resample_stage", "default_cuts", "smc_bound"]

MODES = ldvi.MODES
_MISSING = _missing("an LDVI segment", "smc_ldvi")


def _refuse_other_modes(params_fixed):
    mode = params_fixed[2] if len(params_fixed) == 4 else None
    if mode not in MODES:
        where = ("cmcd_amd.smc_uha" if mode == "MCD_CAIS_UHA_sn" else
                 "cmcd_amd.smc_hais" if len(params_fixed) == 3 else "cmcd_amd.smc")
        raise NotImplementedError(f"cmcd_amd.smc_ldvi runs {MODES[0]} and {MODES[1]} only (this params_fixed: {where})")


def segment(state, k0, k1, params_flat, unflatten, params_fixed, log_prob, eps_schedule=None, grad_clipping=False):
    """Bridges [k0, k1) of the LDVI forward chain, one library call on the current stream; `params_fixed` is `ldvi.initialize`'s.
    `state` is `seeds[N]` at k0 == 0 (the chain then starts from q exactly as `ldvi.bound_forward`), otherwise the state of the
    previous stage, which is left untouched.  -> the state at bridge k1 (see the module text); its `stats` are the five statistics
    over -(wpath + lg).  gmm / funnel / many_gmm on the geffner widths of the forward call only (NotImplementedError otherwise;
    the other modes: `cmcd_amd.smc`, `cmcd_amd.smc_uha`, `cmcd_amd.smc_hais`).  eps_schedule / grad_clipping are accepted for
    the signature and ignored: the mode has neither."""
    _refuse_other_modes(params_fixed)
    desc, lay, use_net = ldvi._plan(unflatten, params_fixed, log_prob)
    k0, k1 = int(k0), int(k1)
    L, dref = _lib.lib(), C.byref(desc)
    return _chain.segment_call(
        state, k0, k1, params_flat, params_fixed[0], True, _MISSING, "seg_ldvi", "no LDVI segment kernel for this configuration",
        False, L.cmcd_segment_ldvi_workspace_bytes, (dref, use_net), (bytes(desc), use_net),
        L.cmcd_bound_segment_ldvi, (dref, C.byref(lay), use_net, k0, k1), log_prob.consts_on)


def smc_bound(seeds, params_flat, unflatten, params_fixed, log_prob, eps_schedule=None, grad_clipping=False, *, groups=1,
              cuts=None, ess_threshold=0.5, seed=0, trace=False):
    """`cmcd_amd.smc_uha.smc_bound` for LDVI: the chain of `ldvi.bound_forward` with resampling stages at the bridges `cuts`.
    Same arguments, same result dict (ln_Z, losses, z, rho, resampled, ess; with trace=True the stages).  With ess_threshold = 0
    nothing is resampled and losses are the single segment [0, K)'s, bit for bit.  No host read."""
    _refuse_other_modes(params_fixed)
    return _chain.drive(segment, True, seeds, params_flat, unflatten, params_fixed, log_prob, eps_schedule, grad_clipping, groups,
                        cuts, ess_threshold, seed, trace)
