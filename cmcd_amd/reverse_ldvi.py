"""The reverse-time chain of LDVI (`MCD_U_a-lp-sn` and its network-free sibling `MCD_U_a-lp`): `reverse_uha.bound_reverse` for
the two modes it refuses.

`bound_reverse` is ONE call of libcmcd_hip.so (cmcd_bound_reverse_ldvi, csrc/cmcd_reverse_ldvi.hip): exact target draws `x[n, dim]`
get a fresh momentum and are pushed through the backward momentum kernels and the inverted leap-frogs of the trained sampler, with
the noise of `seeds[n]`.  w is the functional `ldvi.bound_forward` returns as -loss, on a path drawn from
p(z_K) N(rho_K) prod B_i: mean(w) is the EUBO (with the forward call's ELBO a bracket of ln Z), exp(-w) are the importance weights
of the reverse estimate of 1 / Z (`utils.log_reverse_diagnostics`, `resample.importance_stats` on w).  Against the 2nd-order chain:
no network in the forward kernel (one evaluation per bridge), the scalar step size, no clip of grad log p; the tree's `eta` leaf is
not read.  Nothing here reads a device value back to the host, so the call can be captured into a graph.  The reference has no
counterpart; the arithmetic is written out in include/cmcd_hip.h and restated in float64 in tests/reverse_ldvi_restatement.py.
No CPU fallback.

Not here: lgcp, a cooperative kernel form, sharding.  (Chain segments and the SMC evaluation of these modes: cmcd_amd.smc_ldvi.)"""
import ctypes as C

from . import _chain, _lib
from . import ldvi
from ._chain import eubo_of

__all__ = ["bound_reverse", "compute_reverse_bound"]

MODES = ldvi.MODES


def bound_reverse(seeds, x, params_flat, unflatten, params_fixed, log_prob, eps_schedule=None, grad_clipping=False):
    """`x[n, dim]`, draws from the target, through the reverse-time chain of LDVI with the noise of `seeds[n]`; `params_fixed` is
    `ldvi.initialize`'s.  Returns (w[N] f32, z0[N, dim] f32, rho0[N, dim] f32, stats[5] f64), all device tensors, enqueued
    asynchronously on the current stream; the statistics are taken over l := w.  A non-finite row of x (or one under many_gmm's
    floor of log p) gives w = +inf (its z0 / rho0 rows are meaningless).  gmm / funnel / many_gmm on the geffner widths of the
    forward call only (NotImplementedError otherwise).  eps_schedule / grad_clipping are accepted for the signature and ignored:
    the mode has neither."""
    desc, lay, use_net = ldvi._plan(unflatten, params_fixed, log_prob)
    L, dref = _lib.lib(), C.byref(desc)
    return _chain.reverse_call(
        seeds, x, params_flat, params_fixed[0], True, "rev_ldvi", "no LDVI reverse-chain kernel for this configuration", False,
        L.cmcd_reverse_ldvi_workspace_bytes, (dref, use_net), (bytes(desc), use_net),
        L.cmcd_bound_reverse_ldvi, (dref, C.byref(lay), use_net), log_prob.consts_on)


def compute_reverse_bound(seeds, x, params_flat, unflatten, params_fixed, log_prob, eps_schedule=None, grad_clipping=False):
    """-> (EUBO = mean(w), (w, z0)) of `bound_reverse`: E[w] >= ln Z, the upper half of the bracket whose lower half is
    -ldvi.compute_bound(...)[0].  +inf when a row of x is non-finite or a chain diverged, never NaN."""
    return eubo_of(bound_reverse(seeds, x, params_flat, unflatten, params_fixed, log_prob,
                                 eps_schedule=eps_schedule, grad_clipping=grad_clipping))
