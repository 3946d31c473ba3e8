"""UHA — Hamiltonian AIS on lgcp (d = 1600), `config.boundmode = "UHA"` with `config.model = "lgcp"`: the arithmetic of
`cmcd_amd.hais` on the log-Gaussian Cox process through its own entry points (`cmcd_hais_lgcp_bound_grad`,
cmcd_amd/csrc/cmcd_hais_lgcp.hip: one launch per target evaluation, the product with the prior precision on the matrix cores
and the leap-frog step in its epilogue; include/cmcd_hip.h states the workspace and the kept rows).

Same interface as `cmcd_amd.hais`: `initialize` is `boundingmachine.initialize`, `compute_bound` / `grad_and_loss` have the
signatures `opt.run` and `utils.sample` expect, `params_fixed = (dim, nbridges, lfsteps)`, `nbridges = 0` goes to
`boundingmachine`.  Any other target belongs to `cmcd_amd.hais` (NotImplementedError).  There is no CPU fallback."""
import torch

from . import _lib
from . import boundingmachine as _bm
from .hais import _layout
from ._call import consts_args, _inputs, on_device, _outputs, _workspace, _zero_notrain

initialize = _bm.initialize


def _call(seeds, params_flat, unflatten, params_fixed, log_prob, want_grad, n_total=None):
    dim, nbridges, lfsteps = params_fixed
    if not hasattr(log_prob, "target_id"):
        raise TypeError("log_prob must be a cmcd_amd.model_handler.Target (see load_model)")
    if log_prob.target_id != _lib.TARGET["lgcp"]:
        raise NotImplementedError("cmcd_amd.hais_lgcp runs UHA on lgcp only: use cmcd_amd.hais for target %r" % log_prob.name)
    if nbridges == 0:
        return _bm._call(seeds, params_flat, unflatten, params_fixed, log_prob, want_grad, n_total)
    if log_prob.dim != dim:
        raise ValueError(f"target dim {log_prob.dim} != params_fixed dim {dim}")
    if nbridges < 0 or lfsteps < 1:
        raise ValueError(f"nbridges = {nbridges}, lfsteps = {lfsteps}: need nbridges >= 0 and lfsteps >= 1")
    seeds, n = _inputs(seeds, params_flat)
    L = _lib.lib()
    device = params_flat.device

    def launch(dev_index, stream, capturing):
        nbytes = L.cmcd_hais_lgcp_workspace_bytes(dim, nbridges, lfsteps, n, int(want_grad))
        ws = _workspace(dev_index, device, stream, capturing, nbytes, "hais_lgcp",
                        "no Hamiltonian AIS lgcp kernel for this shape")
        cptr, cnum = consts_args(log_prob.consts_on(device))       # (lgcp always has constants: the counts and the prior)
        losses, z, stats = _outputs(n, dim, device)
        grad = torch.empty_like(params_flat) if want_grad else None
        lay = _layout(unflatten)
        _lib.check(L.cmcd_hais_lgcp_bound_grad(
            dim, nbridges, lfsteps, lay, seeds.data_ptr(), n, params_flat.data_ptr(), params_flat.numel(),
            cptr, cnum, 1.0 / float(n if n_total is None else n_total), ws.data_ptr(), ws.numel(),
            losses.data_ptr(), z.data_ptr(), stats.data_ptr(), grad.data_ptr() if want_grad else None, stream))
        if want_grad:
            _zero_notrain(grad, unflatten)      # leaves outside `trainable` => zero
        return grad, losses, z, stats

    return on_device(device, launch)


def bound_forward(seeds, params_flat, unflatten, params_fixed, log_prob):
    """-> (losses[n], z[n, dim], stats[5] float64): the three outputs of the library call, nothing derived."""
    _, losses, z, stats = _call(seeds, params_flat, unflatten, params_fixed, log_prob, False)
    return losses, z, stats


def compute_bound(seeds, params_flat, unflatten, params_fixed, log_prob):
    """`bm.compute_bound` -> (ratios.mean(), (ratios, z))."""
    _, losses, z, stats = _call(seeds, params_flat, unflatten, params_fixed, log_prob, False)
    return (stats[1] / losses.numel()).to(torch.float32), (losses, z)


def grad_and_loss(seeds, params_flat, unflatten, params_fixed, log_prob, n_total=None):
    """`jax.jit(jax.grad(bm.compute_bound, 1, has_aux=True))` -> (grad_flat, (ratios, z))."""
    grad, losses, z, _ = _call(seeds, params_flat, unflatten, params_fixed, log_prob, True, n_total)
    return grad, (losses, z)
