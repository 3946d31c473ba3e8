"""UHA — Hamiltonian AIS, `config.boundmode = "UHA"`: the reference's plain bounding machine with `nbridges >= 1`
(/root/reference/src/boundingmachine.py:73-111 -> ais_utils.py:7-69 -> momdist.py:13-28) on the GPU through the C ABI
(`cmcd_hais_bound_grad`, cmcd_amd/csrc/cmcd_hais.hip; the arithmetic is written out in include/cmcd_hip.h).

`initialize` is `boundingmachine.initialize` (the reference's parameter tree: `vd`, `eps`, `eta`, `md`, `mgridref_y`, the two
grids); `compute_bound` / `grad_and_loss` have the signatures `opt.run` and `utils.sample` expect, with
`params_fixed = (dim, nbridges, lfsteps)`.  `nbridges = 0` is the mean-field bound and goes to `boundingmachine`.  There is no
CPU fallback; lgcp (d = 1600) runs through `cmcd_amd.hais_lgcp`, a launch sequence with entry points of its own, and is refused here
(NotImplementedError).  The reverse-time chain of this boundmode is `cmcd_amd.reverse_hais`, its chain segments and SMC evaluation
`cmcd_amd.smc_hais` (gmm / funnel / many_gmm; lgcp has whole chains only).  Not here: a cooperative kernel form, sharding."""
import torch

from . import _lib
from . import boundingmachine as _bm
from ._call import consts_args, _inputs, on_device, _outputs, _workspace, _zero_notrain

initialize = _bm.initialize


def _layout(unflatten):
    """The leaf offsets for the library (read-only there), built once per tree: an Unflatten never changes (as `ldvi._plan`)."""
    lay = unflatten.__dict__.get("_hais_layout")
    if lay is not None:
        return lay
    lay = _lib.HaisLayout(vd_mean=unflatten.offset("vd", "mean"), vd_logdiag=unflatten.offset("vd", "logdiag"),
                          eps=unflatten.offset("eps"), eta=unflatten.offset("eta"), md=unflatten.offset("md"),
                          mgridref_y=unflatten.offset("mgridref_y"), gridref_x=unflatten.offset("gridref_x"),
                          target_x=unflatten.offset("target_x"), ngrid=0)
    shape = unflatten.shape("mgridref_y")
    if shape is None:
        raise ValueError("params tree has no mgridref_y leaf (use hais.initialize)")
    lay.ngrid = shape[0] - 1
    unflatten._hais_layout = lay
    return lay


def _call(seeds, params_flat, unflatten, params_fixed, log_prob, want_grad, n_total=None):
    dim, nbridges, lfsteps = params_fixed
    if nbridges == 0:
        return _bm._call(seeds, params_flat, unflatten, params_fixed, log_prob, want_grad, n_total)
    if not hasattr(log_prob, "target_id"):
        raise TypeError("log_prob must be a cmcd_amd.model_handler.Target (see load_model)")
    if log_prob.dim != dim:
        raise ValueError(f"target dim {log_prob.dim} != params_fixed dim {dim}")
    if nbridges < 0 or lfsteps < 1:
        raise ValueError(f"nbridges = {nbridges}, lfsteps = {lfsteps}: need nbridges >= 0 and lfsteps >= 1")
    seeds, n = _inputs(seeds, params_flat)
    L = _lib.lib()
    device = params_flat.device

    def launch(dev_index, stream, capturing):
        nbytes = L.cmcd_hais_workspace_bytes(log_prob.target_id, dim, nbridges, lfsteps, n, int(want_grad))
        ws = _workspace(dev_index, device, stream, capturing, nbytes, "hais",
                        "no Hamiltonian AIS kernel for this target")
        cptr, cnum = consts_args(log_prob.consts_on(device))
        losses, z, stats = _outputs(n, dim, device)
        grad = torch.empty_like(params_flat) if want_grad else None
        lay = _layout(unflatten)
        _lib.check(L.cmcd_hais_bound_grad(
            log_prob.target_id, dim, nbridges, lfsteps, lay,
            seeds.data_ptr(), n, params_flat.data_ptr(), params_flat.numel(), cptr, cnum,
            1.0 / float(n if n_total is None else n_total), ws.data_ptr(), ws.numel(),
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
    """/root/reference/src/boundingmachine.py:107-111 -> (ratios.mean(), (ratios, z))."""
    _, losses, z, stats = _call(seeds, params_flat, unflatten, params_fixed, log_prob, False)
    return (stats[1] / losses.numel()).to(torch.float32), (losses, z)


def grad_and_loss(seeds, params_flat, unflatten, params_fixed, log_prob, n_total=None):
    """`jax.jit(jax.grad(bm.compute_bound, 1, has_aux=True))` (/root/reference/src/main.py:124-126)
    -> (grad_flat, (ratios, z))."""
    grad, losses, z, _ = _call(seeds, params_flat, unflatten, params_fixed, log_prob, True, n_total)
    return grad, (losses, z)
