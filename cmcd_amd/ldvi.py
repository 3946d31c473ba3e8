"""LDVI — `config.boundmode = "MCD_U_a-lp-sn"` (the README's LDVI) and its network-free sibling `"MCD_U_a-lp"`: the reference's
MCD bounding machine on the underdamped chain with an approximate momentum refresh
(/root/reference/src/mcdboundingmachine.py:126-205 -> mcd_utils.py:83-120 -> mcd_under_lp_a.py:6-87) on the GPU through the C ABI
(`cmcd_ldvi_bound_grad`, cmcd_amd/csrc/cmcd_ldvi.hip; the arithmetic is written out in include/cmcd_hip.h).

`initialize` has `mcdboundingmachine.initialize`'s signature.  For `MCD_U_a-lp-sn` the tree is the one the reference builds for
`MCD_CAIS_UHA_sn` as well (score network with rho_dim = dim, mcdboundingmachine.py:82-99), so it is obtained from there and
only the mode string of `params_fixed` differs; `MCD_U_a-lp` has no `sn`.  `compute_bound` / `grad_and_loss` have the signatures
`opt.run` and `utils.sample` expect, with `params_fixed = (dim, nbridges, mode, apply_fun_sn)`.  The mode takes no `eps_schedule`
and no `grad_clipping` (the function body has neither); the tree's `eta` leaf is not read.  There is no CPU fallback; lgcp and
the dds network have no kernel (NotImplementedError).  The reverse-time chain of these modes is `cmcd_amd.reverse_ldvi`, their chain
segments and SMC evaluation `cmcd_amd.smc_ldvi`.  Not here: lgcp, a cooperative kernel form, sharding."""
import ctypes as C

import torch

from . import _lib
from . import mcdboundingmachine as _mcdbm
from ._call import consts_args, _inputs, on_device, _outputs, _workspace, _zero_notrain
from .nn import ScoreNet

MODES = ("MCD_U_a-lp-sn", "MCD_U_a-lp")


def initialize(dim, vdparams=None, nbridges=0, eps=0.01, gamma=10.0, eta=0.5, ngridb=32, mgridref_y=None, trainable=["eps"],
               use_score_nn=True, emb_dim=48, nlayers=3, seed=1, mode="MCD_U_a-lp-sn", nn_arch="dds",
               fully_connected_units=None, device=None):
    """/root/reference/src/mcdboundingmachine.py:11-123 for the two LDVI modes -> (params_flat, unflatten, params_fixed)."""
    if mode not in MODES:
        raise NotImplementedError("Mode not implemented.")
    sn = mode == "MCD_U_a-lp-sn"
    if sn and nn_arch != "geffner":
        raise NotImplementedError(f"nn_arch = {nn_arch!r} is not implemented for {mode} (geffner only)")
    params_flat, unflatten, (d, k, _, spec) = _mcdbm.initialize(
        dim, vdparams=vdparams, nbridges=nbridges, eps=eps, gamma=gamma, eta=eta, ngridb=ngridb, mgridref_y=mgridref_y,
        trainable=trainable, use_score_nn=use_score_nn, emb_dim=emb_dim, nlayers=nlayers, seed=seed,
        mode="MCD_CAIS_UHA_sn" if sn else mode, nn_arch=nn_arch, fully_connected_units=fully_connected_units, device=device)
    return params_flat, unflatten, (d, k, mode, spec)


def _plan(unflatten, params_fixed, log_prob):
    """Validation in the order of the other entry points (mode, target type, target dim; the device comes with the tensors)
    -> (desc, layout, use_net), built once per (unflatten, params_fixed, target)."""
    dim, nbridges, mode, spec = params_fixed
    if mode not in MODES:
        raise NotImplementedError("Mode not implemented.")
    use_net = mode == "MCD_U_a-lp-sn"
    if use_net:
        if not isinstance(spec, ScoreNet):
            raise ValueError("params_fixed[3] must be the ScoreNet returned by initialize()")
        if spec.arch != "geffner":
            raise NotImplementedError(f"nn_arch = {spec.arch!r} is not implemented for {mode} (geffner only)")
    if not hasattr(log_prob, "target_id"):
        raise TypeError("log_prob must be a cmcd_amd.model_handler.Target (see load_model)")
    if log_prob.dim != dim:
        raise ValueError(f"target dim {log_prob.dim} != params_fixed dim {dim}")
    cache = unflatten.__dict__.setdefault("_ldvi_plans", {})
    key = (params_fixed, id(log_prob))
    plan = cache.get(key)
    if plan is None:
        shape = unflatten.shape("mgridref_y")
        if shape is None:
            raise ValueError("params tree has no mgridref_y leaf (use ldvi.initialize)")
        # mode / eps_schedule / grad_clipping / reserved of the descriptor are ignored by the LDVI entry points
        desc = _lib.Desc(dim=dim, nbridges=nbridges, mode=_lib.MODE["MCD_CAIS_UHA_sn"], arch=_lib.ARCH["geffner"],
                         emb_dim=spec.emb_dim if use_net else 0, target=log_prob.target_id, eps_schedule=0, grad_clipping=0,
                         ngrid=shape[0] - 1, reserved=0)
        if use_net:
            lay = _mcdbm._layout(unflatten, spec)
        else:
            lay = _mcdbm._layout_no_net(unflatten)
            lay.gamma = unflatten.offset("gamma")
        plan = cache[key] = (desc, lay, int(use_net))
    return plan


def _call(seeds, params_flat, unflatten, params_fixed, log_prob, want_grad, n_total=None):
    desc, lay, use_net = _plan(unflatten, params_fixed, log_prob)
    dim = params_fixed[0]
    seeds, n = _inputs(seeds, params_flat)
    L = _lib.lib()
    device = params_flat.device

    def launch(dev_index, stream, capturing):
        nbytes = L.cmcd_ldvi_workspace_bytes(C.byref(desc), use_net, n, int(want_grad))
        ws = _workspace(dev_index, device, stream, capturing, nbytes, "ldvi",
                        "no LDVI kernel for this configuration")
        cptr, cnum = consts_args(log_prob.consts_on(device))
        losses, z, stats = _outputs(n, dim, device)
        grad = torch.empty_like(params_flat) if want_grad else None
        _lib.check(L.cmcd_ldvi_bound_grad(
            C.byref(desc), C.byref(lay), use_net, seeds.data_ptr(), n, params_flat.data_ptr(), params_flat.numel(),
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
    """/root/reference/src/mcdboundingmachine.py:183-205 -> (batch_log_elbos.mean(), (batch_log_elbos, z))."""
    _, losses, z, stats = _call(seeds, params_flat, unflatten, params_fixed, log_prob, False)
    return (stats[1] / losses.numel()).to(torch.float32), (losses, z)


def grad_and_loss(seeds, params_flat, unflatten, params_fixed, log_prob, n_total=None):
    """`jax.jit(jax.grad(mcdbm.compute_bound, 1, has_aux=True))` (/root/reference/src/main.py:174-176)
    -> (grad_flat, (batch_log_elbos, z)); `n_total`: the size of the whole batch when this call holds a shard of it."""
    grad, losses, z, _ = _call(seeds, params_flat, unflatten, params_fixed, log_prob, True, n_total)
    return grad, (losses, z)
