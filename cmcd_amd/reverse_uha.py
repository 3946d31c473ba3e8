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

import torch

from . import _lib
from . import mcdboundingmachine as mcdbm
from ._call import check_x, consts_args, _inputs, on_device, _outputs, _workspace

__all__ = ["bound_reverse", "compute_reverse_bound"]

MODE = "MCD_CAIS_UHA_sn"


def bound_reverse(seeds, x, params_flat, unflatten, params_fixed, log_prob, eps_schedule=None, grad_clipping=False):
    """`x[n, dim]`, draws from the target, through the reverse-time chain of `MCD_CAIS_UHA_sn` with the noise of `seeds[n]`.
    Returns (w[N] f32, z0[N, dim] f32, rho0[N, dim] f32, stats[5] f64), all device tensors, enqueued asynchronously on the current
    stream; the statistics are taken over l := w.  A non-finite row of x gives w = +inf (its z0 / rho0 rows are meaningless).
    gmm / funnel / many_gmm only (NotImplementedError otherwise; the overdamped modes: `mcdboundingmachine.bound_reverse`).
    eps_schedule / grad_clipping are accepted for the signature and ignored, as by the forward call of this mode."""
    plan = mcdbm._plan(unflatten, params_fixed, log_prob, eps_schedule, grad_clipping)
    seeds, n = _inputs(seeds, params_flat)
    device, dim = params_flat.device, params_fixed[0]
    check_x(x, n, dim, device)

    def launch(dev_index, stream, capturing):
        nbytes = mcdbm._nbytes(plan, "cmcd_reverse_uha_workspace_bytes", n)
        ws = _workspace(dev_index, device, stream, capturing, nbytes, "rev_uha",
                        "no 2nd-order reverse-chain kernel for this configuration", retire=True)
        cptr, cnum = consts_args(log_prob.consts_on(device))
        w, z0, stats = _outputs(n, dim, device)
        rho0 = torch.empty((n, dim), dtype=torch.float32, device=device)
        _lib.check(_lib.lib().cmcd_bound_reverse_uha(
            C.byref(plan.desc), C.byref(plan.lay), seeds.data_ptr(), x.data_ptr(), n, params_flat.data_ptr(),
            params_flat.numel(), cptr, cnum, ws.data_ptr(), ws.numel(), w.data_ptr(), z0.data_ptr(), rho0.data_ptr(),
            stats.data_ptr(), stream))
        return w, z0, rho0, stats

    return on_device(device, launch)


def compute_reverse_bound(seeds, x, params_flat, unflatten, params_fixed, log_prob, eps_schedule=None, grad_clipping=False):
    """-> (EUBO = mean(w), (w, z0)) of `bound_reverse`: E[w] >= ln Z, the upper half of the bracket whose lower half is
    -compute_bound(...)[0].  +inf when a row of x is non-finite or a chain diverged, never NaN."""
    return mcdbm.eubo_of(bound_reverse(seeds, x, params_flat, unflatten, params_fixed, log_prob,
                                       eps_schedule=eps_schedule, grad_clipping=grad_clipping))
