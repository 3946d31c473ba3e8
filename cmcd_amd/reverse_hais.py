"""The reverse-time chain of UHA (Hamiltonian AIS, `config.boundmode = "UHA"`): `reverse_uha.bound_reverse` for the plain bounding
machine with `nbridges >= 1`.

`bound_reverse` is ONE call of libcmcd_hip.so (cmcd_bound_reverse_hais, csrc/cmcd_reverse_hais.hip): exact target draws
`x[n, dim]` get a fresh momentum r = exp(md) normal(R) and run the forward chain's leap-frogs backwards, the momentum refreshed
between the bridges by the forward rule (it is reversible with respect to N(0, exp(md)^2)), with the noise of `seeds[n]`.  w is the
functional `hais.bound_forward` returns as -loss, on that reversed path: mean(w) is the EUBO (with the forward call's ELBO a bracket
of ln Z), exp(-w) are the importance weights of the reverse estimate of 1 / Z.  Nothing here reads a device value back to the host,
so the call can be captured into a graph.  The reference has no counterpart; the arithmetic is written out in include/cmcd_hip.h
and restated in float64 in tests/reverse_hais_restatement.py.  No CPU fallback.

Not here: lgcp (it has no exact draws), a cooperative kernel form, sharding.  (Chain segments and the SMC evaluation of this
boundmode: cmcd_amd.smc_hais.)"""
from . import _chain, _lib
from . import hais
from ._chain import eubo_of

__all__ = ["bound_reverse", "compute_reverse_bound"]


def bound_reverse(seeds, x, params_flat, unflatten, params_fixed, log_prob, eps_schedule=None, grad_clipping=False):
    """`x[n, dim]`, draws from the target, through the reverse-time chain of UHA with the noise of `seeds[n]`; `params_fixed` is
    `hais.initialize`'s (dim, nbridges, lfsteps).  Returns (w[N] f32, z0[N, dim] f32, rho0[N, dim] f32, stats[5] f64), all device
    tensors, enqueued asynchronously on the current stream; rho0 is the chain's initial momentum, the statistics are taken over
    l := w.  A non-finite row of x (or one under many_gmm's floor of log p) gives w = +inf.  gmm / funnel / many_gmm only
    (NotImplementedError otherwise, lgcp included); nbridges = 0 has no chain (ValueError).  eps_schedule / grad_clipping are
    accepted for the signature and ignored: the mode has neither."""
    dim, nbridges, lfsteps = params_fixed
    if not hasattr(log_prob, "target_id"):
        raise TypeError("log_prob must be a cmcd_amd.model_handler.Target (see load_model)")
    if log_prob.dim != dim:
        raise ValueError(f"target dim {log_prob.dim} != params_fixed dim {dim}")
    if nbridges < 1 or lfsteps < 1:
        raise ValueError(f"nbridges = {nbridges}, lfsteps = {lfsteps}: the reverse chain needs nbridges >= 1 and lfsteps >= 1")
    L, shape = _lib.lib(), (log_prob.target_id, dim, nbridges, lfsteps)
    # (the layout struct is formed in front of the C call, behind the checks of seeds, x and the size query)
    return _chain.reverse_call(
        seeds, x, params_flat, dim, True, "rev_hais", "no Hamiltonian AIS reverse-chain kernel for this target", False,
        L.cmcd_reverse_hais_workspace_bytes, shape, shape,
        L.cmcd_bound_reverse_hais, lambda: (*shape, hais._layout(unflatten)), log_prob.consts_on)


def compute_reverse_bound(seeds, x, params_flat, unflatten, params_fixed, log_prob, eps_schedule=None, grad_clipping=False):
    """-> (EUBO = mean(w), (w, z0)) of `bound_reverse`: E[w] >= ln Z, the upper half of the bracket whose lower half is
    -hais.compute_bound(...)[0].  +inf when a row of x is non-finite or a chain diverged, never NaN."""
    return eubo_of(bound_reverse(seeds, x, params_flat, unflatten, params_fixed, log_prob,
                                 eps_schedule=eps_schedule, grad_clipping=grad_clipping))
