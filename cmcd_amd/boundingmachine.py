"""Host mirror of /root/reference/src/boundingmachine.py for the part the CMCD runs depend on: the
mean-field VI bound (`nbridges = 0`) that /root/reference/src/main.py:82-109 optimises
(`config.pretrain_mfvi`, trainable = ("vd",)) to obtain `vdparams_init` for every MCD mode.

`initialize` reproduces the reference's parameter tree (and so the `params_flat` layout) for any
`nbridges`; `compute_bound` / `grad_and_loss` run on the GPU through the C ABI (`cmcd_mfvi_bound_grad`)
for `nbridges = 0` and raise `NotImplementedError` for `nbridges >= 1`: the UHA chain (ais_utils.evolve, Hamiltonian AIS) is
reached through `cmcd_amd.hais`, whose `initialize` is this module's and whose `compute_bound` / `grad_and_loss` take the same
arguments (`cmcd_hais_bound_grad`)."""
import torch

from . import _lib
from . import variationaldist as vd
from ._call import consts_args, _inputs, on_device, _outputs, _workspace, _zero_notrain
from .mcdboundingmachine import ravel_pytree


def initialize(dim, vdparams=None, nbridges=0, lfsteps=1, eps=0.0, eta=0.5, mdparams=None, ngridb=32,
               mgridref_y=None, trainable=("eps", "eta"), init_sigma=1.0, device=None):
    """/root/reference/src/boundingmachine.py:9-70 -> (params_flat, unflatten, params_fixed = (dim, nbridges, lfsteps))."""
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
    params_train, params_notrain = {}, {}

    def put(name, value):
        (params_train if name in trainable else params_notrain)[name] = value

    put("vd", vdparams if vdparams is not None else vd.initialize(dim, init_sigma=init_sigma))
    put("eps", torch.tensor(float(eps), dtype=torch.float32))
    put("eta", torch.tensor(float(eta), dtype=torch.float32))
    put("md", mdparams if mdparams is not None else torch.zeros(dim, dtype=torch.float32))   # momdist.py:8-10
    if mgridref_y is not None:
        mgridref_y = torch.as_tensor(mgridref_y, dtype=torch.float32)
        ngridb = mgridref_y.shape[0] - 1
    else:
        if nbridges < ngridb:
            ngridb = nbridges
        mgridref_y = torch.ones(ngridb + 1, dtype=torch.float32)
    params_notrain["gridref_x"] = torch.linspace(0, 1, ngridb + 2, dtype=torch.float32)
    params_notrain["target_x"] = torch.linspace(0, 1, nbridges + 2, dtype=torch.float32)[1:-1]
    put("mgridref_y", mgridref_y)
    params_fixed = (dim, nbridges, lfsteps)
    params_flat, unflatten = ravel_pytree((params_train, params_notrain), device=device)
    return params_flat, unflatten, params_fixed


def _call(seeds, params_flat, unflatten, params_fixed, log_prob, want_grad, n_total=None):
    dim, nbridges, _ = params_fixed
    if nbridges >= 1:
        raise NotImplementedError("UHA (nbridges >= 1) is not implemented: only the mean-field bound (nbridges = 0).")
    if not hasattr(log_prob, "target_id"):
        raise TypeError("log_prob must be a cmcd_amd.model_handler.Target (see load_model)")
    if log_prob.dim != dim:
        raise ValueError(f"target dim {log_prob.dim} != params_fixed dim {dim}")
    seeds, n = _inputs(seeds, params_flat)
    L = _lib.lib()
    device = params_flat.device

    def launch(dev_index, stream, capturing):
        nbytes = L.cmcd_mfvi_workspace_bytes(log_prob.target_id, dim, n)
        ws = _workspace(dev_index, device, stream, capturing, nbytes, "mfvi",
                        "no mean-field kernel for this target")
        cptr, cnum = consts_args(log_prob.consts_on(device))
        losses, z, stats = _outputs(n, dim, device)
        grad = torch.empty_like(params_flat) if want_grad else None
        _lib.check(L.cmcd_mfvi_bound_grad(
            log_prob.target_id, dim, unflatten.offset("vd", "mean"), unflatten.offset("vd", "logdiag"),
            seeds.data_ptr(), n, params_flat.data_ptr(), params_flat.numel(), cptr, cnum,
            1.0 / float(n if n_total is None else n_total), ws.data_ptr(), ws.numel(),
            losses.data_ptr(), z.data_ptr(), stats.data_ptr(), grad.data_ptr() if want_grad else None, stream))
        if want_grad:
            _zero_notrain(grad, unflatten)      # "vd" outside `trainable` => zero
        return grad, losses, z, stats

    return on_device(device, launch)


def compute_bound(seeds, params_flat, unflatten, params_fixed, log_prob):
    """/root/reference/src/boundingmachine.py:114-118 -> (ratios.mean(), (ratios, z))."""
    _, losses, z, stats = _call(seeds, params_flat, unflatten, params_fixed, log_prob, False)
    return (stats[1] / losses.numel()).to(torch.float32), (losses, z)


def grad_and_loss(seeds, params_flat, unflatten, params_fixed, log_prob, n_total=None):
    """`jax.jit(jax.grad(bm.compute_bound, 1, has_aux=True))` (/root/reference/src/main.py:87-89)
    -> (grad_flat, (ratios, z))."""
    grad, losses, z, _ = _call(seeds, params_flat, unflatten, params_fixed, log_prob, True, n_total)
    return grad, (losses, z)
