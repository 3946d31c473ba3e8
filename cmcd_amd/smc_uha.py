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
from here, and all four families share one call path and one driver loop (cmcd_amd._chain).  Not here: lgcp, the cooperative
kernel forms, sharding.  (The reverse-time chain of this mode: cmcd_amd.reverse_uha.)"""
import ctypes as C

from . import _chain, _lib
from . import mcdboundingmachine as mcdbm
from ._chain import default_cuts, losses_of

__all__ = ["STATE_FIELDS", "segment", "losses_of", "resample_stage", "default_cuts", "smc_bound"]

STATE_FIELDS = ("z", "rho", "wpath", "lg", "key")
MODE = "MCD_CAIS_UHA_sn"


def _missing(what="a 2nd-order segment", module="smc_uha"):
    """The TypeError text of this module's, smc_ldvi's and smc_hais's segment for what is no state with momentum."""
    return (f"{what} with k0 > 0 starts from the state dict an earlier {module}.segment (or resample_stage) returned: z, rho, wpath "
            "and key")


_MISSING = _missing()


def segment(state, k0, k1, params_flat, unflatten, params_fixed, log_prob, eps_schedule=None, grad_clipping=False):
    """Bridges [k0, k1) of the 2nd-order forward chain, one library call on the current stream.  `state` is `seeds[N]` at k0 == 0
    (the chain then starts from q exactly as `bound_forward`), otherwise the state of the previous stage, which is left untouched.
    -> the state at bridge k1 (see the module text); its `stats` are the five statistics over -(wpath + lg).
    `MCD_CAIS_UHA_sn` on gmm / funnel / many_gmm only (NotImplementedError otherwise; the overdamped modes: `cmcd_amd.smc`).
    eps_schedule / grad_clipping are accepted for the signature and ignored, as by the forward call of this mode."""
    plan = mcdbm._plan(unflatten, params_fixed, log_prob, eps_schedule, grad_clipping)
    if params_fixed[2] != MODE:
        raise NotImplementedError(f"cmcd_amd.smc_uha runs {MODE} only (boundmode {params_fixed[2]!r}: cmcd_amd.smc)")
    k0, k1 = int(k0), int(k1)
    L, desc = _lib.lib(), C.byref(plan.desc)
    return _chain.segment_call(
        state, k0, k1, params_flat, params_fixed[0], True, _MISSING, "seg_uha", "no 2nd-order segment kernel for this configuration",
        True, L.cmcd_segment_uha_workspace_bytes, (desc,), plan.desc_b,
        L.cmcd_bound_segment_uha, (desc, C.byref(plan.lay), k0, k1), log_prob.consts_on)


def resample_stage(state, groups=1, ess_threshold=0.5, seed=0):
    """`cmcd_amd.smc.resample_stage` for the state with momentum: same trigger, same ln Z column, same restart rule
    (wpath_j = -lg[a_j]); a resampled group takes z AND rho from its ancestors — ONE resampling launch on the rows [z | rho] of
    width 2 dim.  KEYS STAY WITH THEIR SLOT.  Every other group is passed through unchanged (identity ancestors).
    -> (new state, {"resampled"[groups] bool, "ess"[groups], "ln_Z_increment"[groups] f64, "ancestors"[N] int64})."""
    return _chain.resample_stage(state, groups, ess_threshold, seed, momentum=True)


def smc_bound(seeds, params_flat, unflatten, params_fixed, log_prob, eps_schedule=None, grad_clipping=False, *, groups=1,
              cuts=None, ess_threshold=0.5, seed=0, trace=False):
    """`cmcd_amd.smc.smc_bound` for `MCD_CAIS_UHA_sn`: the chain of `bound_forward` with resampling stages at the bridges `cuts`.
    Same arguments, same result dict (ln_Z, losses, z, resampled, ess) plus "rho"[N, dim], the final momenta; with trace=True the
    stages carry {"k", "wpath", "lg", "ancestors"} as there.  With ess_threshold = 0 nothing is resampled and losses are the single
    segment [0, K)'s, bit for bit.  Each segment runs the prep launch and evaluates the target at its first state again.  No host
    read."""
    return _chain.drive(segment, True, seeds, params_flat, unflatten, params_fixed, log_prob, eps_schedule, grad_clipping, groups,
                        cuts, ess_threshold, seed, trace)
