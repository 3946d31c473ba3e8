"""The reverse-time chain of 2nd-order CMCD (`MCD_CAIS_UHA_sn`): `mcdboundingmachine.bound_reverse` for the mode it refuses.

`bound_reverse` is ONE call of libcmcd_hip.so (cmcd_bound_reverse_uha, csrc/cmcd_reverse_uha.hip): exact target draws `x[n, dim]`
get a fresh momentum and are pushed through the backward momentum kernels and the inverted leap-frogs of the trained sampler, with
the noise of `seeds[n]`.  w is the functional `bound_forward` returns as -loss in this mode, on a path drawn from
p(z_K) N(rho_K) prod B_i: mean(w) is the EUBO (with the forward call's ELBO a bracket of ln Z), exp(-w) are the importance weights
of the reverse estimate of 1 / Z (`utils.log_reverse_diagnostics`, `resample.importance_stats` on w).  Nothing here reads a device
value back to the host, so the call can be captured into a graph.  The reference has no counterpart; the arithmetic is written out
in include/cmcd_hip.h and restated in float64 NumPy in tests/reverse_uha_restatement.py.  No CPU fallback.

LDVI and the UHA boundmode have reverse chains of their own (`cmcd_amd.reverse_ldvi`, `cmcd_amd.reverse_hais`) and chain segments of
their own (`cmcd_amd.smc_ldvi`, `cmcd_amd.smc_hais`).  Not here: lgcp, a cooperative kernel form, sharding."""
import ctypes as C

from . import _chain, _lib
from . import mcdboundingmachine as mcdbm

__all__ = ["bound_reverse", "compute_reverse_bound"]

MODE = "MCD_CAIS_UHA_sn"


def bound_reverse(seeds, x, params_flat, unflatten, params_fixed, log_prob, eps_schedule=None, grad_clipping=False):
    """`x[n, dim]`, draws from the target, through the reverse-time chain of `MCD_CAIS_UHA_sn` with the noise of `seeds[n]`.
    Returns (w[N] f32, z0[N, dim] f32, rho0[N, dim] f32, stats[5] f64), all device tensors, enqueued asynchronously on the current
    stream; the statistics are taken over l := w.  A non-finite row of x gives w = +inf (its z0 / rho0 rows are meaningless).
    gmm / funnel / many_gmm only (NotImplementedError otherwise; the overdamped modes: `mcdboundingmachine.bound_reverse`).
    eps_schedule / grad_clipping are accepted for the signature and ignored, as by the forward call of this mode."""
    plan = mcdbm._plan(unflatten, params_fixed, log_prob, eps_schedule, grad_clipping)
    L, desc = _lib.lib(), C.byref(plan.desc)
    return _chain.reverse_call(
        seeds, x, params_flat, params_fixed[0], True, "rev_uha", "no 2nd-order reverse-chain kernel for this configuration", True,
        L.cmcd_reverse_uha_workspace_bytes, (desc,), plan.desc_b, L.cmcd_bound_reverse_uha, (desc, C.byref(plan.lay)),
        log_prob.consts_on)


def compute_reverse_bound(seeds, x, params_flat, unflatten, params_fixed, log_prob, eps_schedule=None, grad_clipping=False):
    """-> (EUBO = mean(w), (w, z0)) of `bound_reverse`: E[w] >= ln Z, the upper half of the bracket whose lower half is
    -compute_bound(...)[0].  +inf when a row of x is non-finite or a chain diverged, never NaN."""
    return _chain.eubo_of(bound_reverse(seeds, x, params_flat, unflatten, params_fixed, log_prob,
                                        eps_schedule=eps_schedule, grad_clipping=grad_clipping))
