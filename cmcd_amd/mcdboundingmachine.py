"""The drop-in boundary: `initialize`, `compute_bound`, `compute_bound_var`.

Same names, positional signatures and return structure as
/root/reference/src/mcdboundingmachine.py:11-28,183-231, with torch tensors on a ROCm device in
place of jax arrays and a `Target` descriptor (cmcd_amd.model_handler) in place of the traceable
`log_prob` callable.  All arithmetic of the path runs in libcmcd_hip.so (include/cmcd_hip.h);
there is no CPU fallback.
"""
import ctypes as C
import weakref
from collections import namedtuple

import torch

from . import _chain, _lib
from . import variationaldist as vd
from ._call import (PREP_CALLS, fixed_parameters,      # noqa: F401  (these two, and _outputs, are read through this module)
                    _fixed, _inputs, _outputs, _prepared, _workspace, _zero_notrain, consts_args, on_device)
from ._chain import eubo_of      # noqa: F401  (its home is _chain; the reverse modules and callers read it here too)
from .nn import ScoreNet, initialize_network

_SN_MODES = ["MCD_ULA_sn", "MCD_U_e-lp-sna", "MCD_U_a-lp-sna", "MCD_CAIS_sn", "MCD_CAIS_var_sn"]
_SUPPORTED = ("MCD_CAIS_sn", "MCD_CAIS_var_sn", "MCD_ULA", "MCD_ULA_sn", "MCD_CAIS_UHA_sn")


# --------------------------------------------------------------------------- ravel_pytree
def _flatten(tree, prefix=()):
    """Leaves in jax tree order: dict keys sorted, sequences in order."""
    if isinstance(tree, dict):
        for k in sorted(tree):
            yield from _flatten(tree[k], prefix + (k,))
    elif isinstance(tree, (list, tuple)):
        for i, v in enumerate(tree):
            yield from _flatten(v, prefix + (i,))
    else:
        yield prefix, tree


def _rebuild(tree, leaves, prefix=()):
    if isinstance(tree, dict):
        return {k: _rebuild(tree[k], leaves, prefix + (k,)) for k in tree}
    if isinstance(tree, (list, tuple)):
        return type(tree)(_rebuild(v, leaves, prefix + (i,)) for i, v in enumerate(tree))
    return leaves[prefix]


class Unflatten:
    """Callable inverse of the flattening; also records where each leaf sits (`.layout`)."""

    def __init__(self, tree):
        self._tree = tree
        self.layout = {}
        off = 0
        for path, leaf in _flatten(tree):
            shape = tuple(torch.as_tensor(leaf).shape)
            numel = 1
            for s in shape:
                numel *= s
            self.layout[path] = (off, shape)
            off += numel
        self.size = off

    def __call__(self, params_flat):
        leaves = {p: params_flat[o:o + _numel(s)].reshape(s) for p, (o, s) in self.layout.items()}   # _numel(()) == 1
        return _rebuild(self._tree, leaves)

    def offset(self, *path):
        """Offset of a leaf, searched in (params_train, params_notrain)."""
        for root in (0, 1):
            if (root,) + path in self.layout:
                return self.layout[(root,) + path][0]
        return -1

    def shape(self, *path):
        for root in (0, 1):
            if (root,) + path in self.layout:
                return self.layout[(root,) + path][1]
        return None

    def __hash__(self):
        return id(self)


def _numel(shape):
    n = 1
    for s in shape:
        n *= s
    return n


def ravel_pytree(tree, device=None):
    un = Unflatten(tree)
    flat = torch.cat([torch.as_tensor(leaf, dtype=torch.float32).reshape(-1) for _, leaf in _flatten(tree)])
    if device is not None:
        flat = flat.to(device)
    return flat.contiguous(), un


# --------------------------------------------------------------------------- initialize
def initialize(
    dim,
    vdparams=None,
    nbridges=0,
    eps=0.01,
    gamma=10.0,
    eta=0.5,
    ngridb=32,
    mgridref_y=None,
    trainable=["eps"],
    use_score_nn=True,
    emb_dim=48,
    nlayers=3,
    seed=1,
    mode="MCD_U_lp-e",
    nn_arch="dds",
    fully_connected_units=None,
    device=None,
):
    """/root/reference/src/mcdboundingmachine.py:11-123.  Returns
    (params_flat, unflatten, params_fixed) with params_fixed = (dim, nbridges, mode, apply_fun_sn).
    `device` (extra, keyword-only in practice) defaults to the current ROCm device."""
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
    params_train, params_notrain = {}, {}

    def put(name, value):
        (params_train if name in trainable else params_notrain)[name] = value

    put("vd", vdparams if vdparams is not None else vd.initialize(dim))
    put("eps", torch.tensor(float(eps), dtype=torch.float32))
    put("gamma", torch.tensor(float(gamma), dtype=torch.float32))
    put("eta", torch.tensor(float(eta), dtype=torch.float32))

    if mode in _SN_MODES:
        init_fun_sn, apply_fun_sn = initialize_network(
            dim, emb_dim, nbridges, nlayers=nlayers, nn_arch=nn_arch,
            fully_connected_units=fully_connected_units)
        params_train["sn"] = init_fun_sn(seed, None)[1]
    elif mode == "MCD_CAIS_UHA_sn":
        # score network with rho_dim = dim: its input is concat(z, rho)   (:82-98)
        init_fun_sn, apply_fun_sn = initialize_network(
            dim, emb_dim, nbridges, rho_dim=dim, nlayers=nlayers, nn_arch=nn_arch,
            fully_connected_units=fully_connected_units)
        params_train["sn"] = init_fun_sn(seed, None)[1]
    elif mode in ["MCD_U_a-lp-sn", "MCD_U_ea-lp-sn", "MCD_U_a-nv-sn"]:
        raise NotImplementedError("Mode not implemented.")  # the other momentum modes: outside the hot path
    else:
        apply_fun_sn = None

    # betas = interp over the normalised cumulative mgridref_y   (:104-118)
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

    params_fixed = (dim, nbridges, mode, apply_fun_sn)
    params_flat, unflatten = ravel_pytree((params_train, params_notrain), device=device)
    return params_flat, unflatten, params_fixed


# --------------------------------------------------------------------------- the HIP call
# Kernel variant handed to the library in cmcd_desc.reserved: 0 = auto (library heuristic),
# 1 = wave-per-tile kernel, 2 = CU-cooperative kernel (library picks the tile), 3 / 4 = cooperative on 16- / 8-particle
# tiles.  For tests / benchmarking only.
KERNEL_VARIANT = int(__import__("os").environ.get("CMCD_KERNEL_VARIANT", "0"))

# Prepared tables for the whole process, without a `with fixed_parameters():` (see _call._prepared).  Read by bound_forward
# at call time as THIS module's attribute: benchmarks and tests assign it here.
PREP_CACHE = __import__("os").environ.get("CMCD_PREP_CACHE", "0") == "1"


def _layout(unflatten, spec):
    """Leaf offsets of `params_flat` for the library (read-only there).  An Unflatten never changes after construction,
    so the struct is built once per (unflatten, net) — twenty dictionary searches per call are host time that a
    K = 8 launch sequence (30 us on the GPU) does not hide."""
    cache = unflatten.__dict__.setdefault("_lay_cache", {})
    lay = cache.get(spec)
    if lay is None:
        lay = cache[spec] = _build_layout(unflatten, spec)
    return lay


def _build_layout(unflatten, spec):
    lay = _lib.Layout(*([-1] * len(_lib.LAYOUT_FIELDS)))
    o = unflatten.offset
    lay.vd_mean, lay.vd_logdiag = o("vd", "mean"), o("vd", "logdiag")
    lay.eps, lay.mgridref_y, lay.gamma = o("eps"), o("mgridref_y"), o("gamma")
    if spec.arch == "geffner":
        lay.g_emb, lay.g_factor = o("sn", "emb"), o("sn", "factor_sn")
        lay.g_w1, lay.g_b1 = o("sn", "nn", 0, 0), o("sn", "nn", 0, 1)
        lay.g_w2, lay.g_b2 = o("sn", "nn", 1, 0), o("sn", "nn", 1, 1)
        lay.g_w3, lay.g_b3 = o("sn", "nn", 2, 0), o("sn", "nn", 2, 1)
    else:
        lay.d_phase = o("sn", "drift_net", "timestep_phase")
        for i, (wn, bn) in enumerate((("d_tw1", "d_tb1"), ("d_tw2", "d_tb2"), ("d_sw1", "d_sb1"), ("d_sw2", "d_sb2"))):
            mod = "drift_net/~/linear" + ("" if i == 0 else f"_{i}")
            setattr(lay, wn, o("sn", mod, "w"))
            setattr(lay, bn, o("sn", mod, "b"))
        lay.d_sw3, lay.d_sb3 = o("sn", "drift_net/~/linear_zero", "w"), o("sn", "drift_net/~/linear_zero", "b")
    return lay


def _layout_no_net(unflatten):
    lay = _lib.Layout(*([-1] * len(_lib.LAYOUT_FIELDS)))
    o = unflatten.offset
    lay.vd_mean, lay.vd_logdiag = o("vd", "mean"), o("vd", "logdiag")
    lay.eps, lay.mgridref_y = o("eps"), o("mgridref_y")
    return lay


_plans = {}      # what one call needs besides its tensors, per (parameter tree, net, mode, target, flags): see _plan
_Plan = namedtuple("_Plan", "unflatten_ref target_ref desc lay desc_b lay_b spec nbytes_of")


def _plan(unflatten, params_fixed, log_prob, eps_schedule, grad_clipping):
    """The descriptor, the layout struct and their byte images for one (unflatten, params_fixed, target, static flags): built
    once, looked up per call, by every entry point of this module — the one place that validates params_fixed / the target
    and builds a cmcd_desc.  A forward call of the smallest configuration is 18 us of GPU time; building two ctypes structs,
    their byte keys and twenty dictionary searches per call made the HOST the bound there (29 us per call, r05
    tools/probes/host_overhead.py).  `nbytes_of` holds the workspace sizes the library reported for this descriptor
    (see _nbytes)."""
    key = (id(unflatten), params_fixed, id(log_prob), eps_schedule, bool(grad_clipping), KERNEL_VARIANT)
    plan = _plans.get(key)
    if plan is not None and plan[0]() is unflatten and plan[1]() is log_prob:
        return plan
    dim, nbridges, mode, spec = params_fixed
    if mode not in _SUPPORTED:
        raise NotImplementedError("Mode not implemented.")  # same text as mcd_utils.py:190
    if mode == "MCD_ULA":
        spec = ScoreNet("dds", dim, 64, 0, 64)   # placeholder: MCD_ULA has no network (apply_fun_sn is None)
    elif not isinstance(spec, ScoreNet):
        raise ValueError("params_fixed[3] must be the ScoreNet returned by initialize()")
    if not hasattr(log_prob, "target_id"):
        raise TypeError("log_prob must be a cmcd_amd.model_handler.Target (see load_model)")
    if log_prob.dim != dim:
        raise ValueError(f"target dim {log_prob.dim} != params_fixed dim {dim}")
    sched = eps_schedule if eps_schedule in _lib.EPS_SCHEDULE else None   # the reference falls through to constant eps (mcd_cais.py:58-59)
    desc = _lib.Desc(dim=dim, nbridges=nbridges, mode=_lib.MODE[mode], arch=_lib.ARCH[spec.arch],
                     emb_dim=spec.emb_dim, target=log_prob.target_id,
                     eps_schedule=_lib.EPS_SCHEDULE[sched], grad_clipping=int(bool(grad_clipping)),
                     ngrid=unflatten.shape("mgridref_y")[0] - 1, reserved=KERNEL_VARIANT)
    lay = _layout(unflatten, spec) if mode != "MCD_ULA" else _layout_no_net(unflatten)
    plan = _Plan(weakref.ref(unflatten), weakref.ref(log_prob), desc, lay, bytes(desc), bytes(lay), spec, {})
    while len(_plans) > 256:
        _plans.pop(next(iter(_plans)))
    _plans[key] = plan
    return plan


def _nbytes(plan, query, n, grad_item=None):
    """What the library's size query `query` (cmcd_workspace_bytes, cmcd_grad_workspace_bytes,
    cmcd_bound_grad_workspace_bytes) answers for the plan's descriptor and n particles, asked once per (query, n, grad_item).
    The two gradient sizes depend on the CMCD_GRAD_ITEM override: the gradient entry points pass the value in force (what
    _lib.sync_grad_item_override() returns) and it is PART OF THE KEY, so a size cached under one setting is never used
    under another.  An answer <= 0 (no kernel; the caller raises) is not kept."""
    key = (query, n, grad_item)
    nbytes = plan.nbytes_of.get(key)
    if nbytes is None:
        nbytes = getattr(_lib.lib(), query)(C.byref(plan.desc), n)
        if nbytes > 0 and len(plan.nbytes_of) < 64:
            plan.nbytes_of[key] = nbytes
    return nbytes


def bound_forward(seeds, params_flat, unflatten, params_fixed, log_prob, eps_schedule=None, grad_clipping=False):
    """One launch sequence of the hot path.  Returns (losses[N] f32, z[N,dim] f32, stats[5] f64),
    all device tensors, enqueued asynchronously on the current stream."""
    plan = _plan(unflatten, params_fixed, log_prob, eps_schedule, grad_clipping)
    _, _, desc, lay, desc_b, lay_b, spec, _ = plan
    seeds, n = _inputs(seeds, params_flat)
    L = _lib.lib()
    device = params_flat.device

    def launch(dev_index, stream, capturing):
        nbytes = _nbytes(plan, "cmcd_workspace_bytes", n)
        if nbytes <= 0:
            _lib.check(-2 if "not implemented" in _lib.last_error() or "no kernel" in _lib.last_error() else -1)
        ws = _workspace(dev_index, device, stream, capturing, nbytes, "")
        consts = log_prob.consts_on(device)
        cptr, cnum = consts_args(consts)
        losses, z, stats = _outputs(n, params_fixed[0], device)
        # the tables this workspace holds: formed by the previous call from exactly these inputs?  (see _call._prepared)
        # `slot` names the buffer on EVERY call — in or out of fixed_parameters(), capturing or not — because every call
        # overwrites the buffer's tables and must therefore retire whatever claim an earlier call left on it (r04 advisor:
        # with the slot computed inside the context only, `with fixed: f(P)`; `f(Q)`; `with fixed: f(P)` ran P on Q's tables)
        slot = (dev_index, ws.data_ptr())
        key = None
        if (PREP_CACHE or getattr(_fixed, "depth", 0) > 0) and not capturing:
            key = (params_flat.data_ptr(), params_flat._version, params_flat.numel(), n, desc_b, lay_b, spec,
                   None if consts is None else (cptr, consts._version, cnum))
        # (key, weak references to the very tensor OBJECTS the tables were formed from): an address and a version counter
        # alone do not identify a tensor — the caching allocator hands a freed tensor's address to the next one of the same
        # size, whose counter starts at the same value (r04: two parameter sets of one test module collided exactly so)
        hit = False
        ent = _prepared.get(slot) if key is not None else None
        if ent is not None and ent[0] == key and ent[1]() is params_flat and (consts is None or ent[2]() is consts):
            hit = True
        fn = L.cmcd_bound_forward_prepared if hit else L.cmcd_bound_forward
        _prepared.pop(slot, None)        # unconditionally: this launch rewrites (or, on an error, may have rewritten) the tables
        PREP_CALLS["prepared" if hit else "full"] += 1
        _lib.check(fn(
            C.byref(desc), C.byref(lay), seeds.data_ptr(), n, params_flat.data_ptr(), params_flat.numel(), cptr, cnum,
            ws.data_ptr(), ws.numel(), losses.data_ptr(), z.data_ptr(), stats.data_ptr(), stream))
        if key is not None:
            _prepared[slot] = (key, weakref.ref(params_flat), weakref.ref(consts) if consts is not None else None)
            while len(_prepared) > 64:
                _prepared.pop(next(iter(_prepared)))
        return losses, z, stats

    return on_device(device, launch)


def bound_reverse(seeds, x, params_flat, unflatten, params_fixed, log_prob, eps_schedule=None, grad_clipping=False):
    """The reverse-time chain (include/cmcd_hip.h: cmcd_bound_reverse): `x[n, dim]`, draws from the target, pushed through the
    backward kernels of the sampler with the noise of `seeds[n]`.  Returns (w[N] f32, z0[N, dim] f32, stats[5] f64), all
    device tensors, enqueued asynchronously on the current stream: w is the functional `bound_forward` returns as -loss, on a
    path drawn from the target's side; the statistics are taken over l := w.  A non-finite row of x gives w = +inf.
    The reference has no such call.  Overdamped modes on gmm / funnel / many_gmm only (NotImplementedError otherwise)."""
    plan = _plan(unflatten, params_fixed, log_prob, eps_schedule, grad_clipping)
    L, desc = _lib.lib(), C.byref(plan.desc)
    return _chain.reverse_call(
        seeds, x, params_flat, params_fixed[0], False, "rev", "no reverse-chain kernel for this configuration", True,
        L.cmcd_reverse_workspace_bytes, (desc,), plan.desc_b, L.cmcd_bound_reverse, (desc, C.byref(plan.lay)), log_prob.consts_on)


def compute_reverse_bound(seeds, x, params_flat, unflatten, params_fixed, log_prob, eps_schedule=None, grad_clipping=False):
    """-> (EUBO = mean(w), (w, z0)) of `bound_reverse`: E_P[w] >= ln Z, the upper half of the bracket whose lower half is
    -compute_bound(...)[0].  +inf when a row of x is non-finite or a chain diverged, never NaN."""
    return eubo_of(bound_reverse(seeds, x, params_flat, unflatten, params_fixed, log_prob,
                                 eps_schedule=eps_schedule, grad_clipping=grad_clipping))


def compute_bound(seeds, params_flat, unflatten, params_fixed, log_prob, eps_schedule=None, grad_clipping=False):
    """/root/reference/src/mcdboundingmachine.py:183-205 -> (mean(losses), (losses, z))."""
    losses, z, stats = bound_forward(seeds, params_flat, unflatten, params_fixed, log_prob,
                                     eps_schedule=eps_schedule, grad_clipping=grad_clipping)
    mean = (stats[1] / losses.numel()).to(torch.float32)
    return mean, (losses, z)


def compute_bound_var(seeds, params_flat, unflatten, params_fixed, log_prob, eps_schedule=None,
                      grad_clipping=False, ln_Z_correction=False):
    """/root/reference/src/mcdboundingmachine.py:208-231 -> (clip(var(losses, ddof=0), +-1e7), (losses, z)).
    `ln_Z_correction` is accepted and unused, as in the reference (:216)."""
    losses, z, stats = bound_forward(seeds, params_flat, unflatten, params_fixed, log_prob,
                                     eps_schedule=eps_schedule, grad_clipping=grad_clipping)
    n = losses.numel()
    mean = stats[1] / n
    var = stats[2] / n - mean * mean  # inf - inf = nan, which clip passes through like jnp.clip
    return torch.clamp(var, -1e7, 1e7).to(torch.float32), (losses, z)


def ln_z_from_stats(stats, n):
    """logsumexp(-losses) - log n (/root/reference/src/utils.py:233-235) from the statistics vector."""
    return stats[3] + torch.log(stats[4]) - torch.log(torch.tensor(float(n), dtype=torch.float64, device=stats.device))


def compute_log_var_grad(seeds, params_flat, unflatten, params_fixed, log_prob, eps_schedule=None,
                         grad_clipping=False, n_total=None, stats_total=None):
    """Value-and-gradient of `compute_bound_var`: what the reference builds as
    `jax.jit(jax.grad(compute_bound_fn, 1, has_aux=True))` (/root/reference/src/main.py:161-176) and calls as
    `grad, (loss, z) = grad_and_loss(seeds, params_flat, unflatten, params_fixed, log_prob_model)`
    (/root/reference/src/opt.py:97-99).  Returns (grad_flat, (losses, z)); `grad_flat` has the layout of
    `params_flat` (zeros for leaves the loss does not reach).  `MCD_CAIS_var_sn` only: its per-step
    `stop_gradient` (/root/reference/src/mcd_cais_var.py:59,79) makes the gradient local per bridge, which
    is what the HIP kernel exploits.  Multi-GPU: pass the global particle count `n_total` and `stats_total` —
    the merged statistics, or a callable `local_stats -> merged_stats` that runs the all-gather between the
    forward and the gradient launch — and all-reduce the returned gradient."""
    if params_fixed[2] != "MCD_CAIS_var_sn":
        raise NotImplementedError("Mode not implemented.")
    plan = _plan(unflatten, params_fixed, log_prob, eps_schedule, grad_clipping)
    seeds, n = _inputs(seeds, params_flat)
    L = _lib.lib()
    device = params_flat.device

    def launch(dev_index, stream, capturing):
        desc, lay = C.byref(plan.desc), C.byref(plan.lay)
        nbytes = _nbytes(plan, "cmcd_grad_workspace_bytes", n, _lib.sync_grad_item_override())
        ws = _workspace(dev_index, device, stream, capturing, nbytes, "grad",
                        "no gradient kernel for this configuration")
        cptr, cnum = consts_args(log_prob.consts_on(device))
        losses, z, stats = _outputs(n, params_fixed[0], device)
        omega = torch.empty(n, dtype=torch.float32, device=device)
        grad = torch.empty_like(params_flat)
        # forward on the gradient workspace: the per-call tables (and, for small batches, the trajectory) stay
        # there for the gradient call, so the chain runs once
        _lib.check(L.cmcd_bound_var_forward(
            desc, lay, seeds.data_ptr(), n, params_flat.data_ptr(), params_flat.numel(),
            cptr, cnum, ws.data_ptr(), ws.numel(), losses.data_ptr(), z.data_ptr(), stats.data_ptr(), stream))
        st = stats if stats_total is None else stats_total
        if callable(st):   # multi-GPU: the caller merges the local statistics across ranks here
            st = st(stats)
        _lib.check(L.cmcd_vargrad_weights(losses.data_ptr(), st.data_ptr(), n, n if n_total is None else int(n_total),
                                          omega.data_ptr(), stream))
        _lib.check(L.cmcd_bound_var_grad_kept(
            desc, lay, seeds.data_ptr(), n, params_flat.data_ptr(), params_flat.numel(),
            cptr, cnum, omega.data_ptr(), ws.data_ptr(), ws.numel(), grad.data_ptr(), stream))
        _zero_notrain(grad, unflatten)
        return grad, (losses, z)

    return on_device(device, launch)


def compute_bound_grad(seeds, params_flat, unflatten, params_fixed, log_prob, eps_schedule=None,
                       grad_clipping=False, n_total=None, return_stats=False):
    """Value-and-gradient of `compute_bound` for `MCD_CAIS_sn`: the reference's
    `jax.jit(jax.grad(compute_bound, 1, has_aux=True))` (/root/reference/src/main.py:174-176), called as
    `grad, (loss, z) = grad_and_loss(seeds, params_flat, unflatten, params_fixed, log_prob_model)`
    (/root/reference/src/opt.py:97-99).  No stop_gradient in this mode (/root/reference/src/mcd_cais.py:46-89):
    the gradient is the full reparameterised one, back through every z_i.  One library call runs the forward
    launch sequence (keeping z_0..z_K in the workspace) and the reverse sweep.
    Returns (grad_flat, (losses, z)) [+ stats with return_stats]; multi-GPU: pass the global particle count
    as `n_total` and all-reduce the returned gradient."""
    # the two overdamped baselines and 2nd-order CMCD (no stop_gradient either) take the same call
    if params_fixed[2] not in ("MCD_CAIS_sn", "MCD_ULA_sn", "MCD_ULA", "MCD_CAIS_UHA_sn"):
        raise NotImplementedError("Mode not implemented.")
    plan = _plan(unflatten, params_fixed, log_prob, eps_schedule, grad_clipping)
    seeds, n = _inputs(seeds, params_flat)
    L = _lib.lib()
    device = params_flat.device

    def launch(dev_index, stream, capturing):
        nbytes = _nbytes(plan, "cmcd_bound_grad_workspace_bytes", n, _lib.sync_grad_item_override())
        ws = _workspace(dev_index, device, stream, capturing, nbytes, "bptt",
                        "no gradient kernel for this configuration")
        cptr, cnum = consts_args(log_prob.consts_on(device))
        losses, z, stats = _outputs(n, params_fixed[0], device)
        grad = torch.empty_like(params_flat)
        _lib.check(L.cmcd_bound_grad(
            C.byref(plan.desc), C.byref(plan.lay), seeds.data_ptr(), n, params_flat.data_ptr(), params_flat.numel(),
            cptr, cnum, 1.0 / float(n if n_total is None else n_total), ws.data_ptr(), ws.numel(),
            losses.data_ptr(), z.data_ptr(), stats.data_ptr(), grad.data_ptr(), stream))
        _zero_notrain(grad, unflatten)
        if return_stats:
            return grad, (losses, z), stats
        return grad, (losses, z)

    return on_device(device, launch)


def make_grad_and_loss(boundmode, eps_schedule=None, grad_clipping=False):
    """The pair the reference's driver builds per run (/root/reference/src/main.py:161-176):
    `grad_and_loss = jit(grad(compute_bound_fn, 1, has_aux=True))`, `loss_fn = jit(compute_bound_fn)`, with
    `compute_bound_var` when "var" is in the boundmode and `compute_bound` otherwise.
    -> (grad_and_loss, loss_fn), both taking (seeds, params_flat, unflatten, params_fixed, log_prob_model)."""
    from functools import partial
    kw = dict(eps_schedule=eps_schedule, grad_clipping=grad_clipping)
    if "var" in boundmode:
        return partial(compute_log_var_grad, **kw), partial(compute_bound_var, **kw)
    return partial(compute_bound_grad, **kw), partial(compute_bound, **kw)
