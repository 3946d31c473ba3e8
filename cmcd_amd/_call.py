"""What every Python entry point of libcmcd_hip.so does around its own C call: the tensor checks, the device and stream of
the call, its scratch buffer and the claim on prepared tables that buffer may carry.  An entry point checks its tensors
(`_inputs`, `check_x`), then hands `on_device` a body that takes the buffer (`_workspace`: the refusal of a size query, the LRU,
the retired claim), the constants (`consts_args`) and the outputs (`_outputs`) and spells out its own C call.  Nothing here
knows a mode, a target or a descriptor.

The eight reverse-chain and chain-segment entry points go through one more layer, `_chain` (`segment_call`, `reverse_call`): it
makes these calls in this order for them — tensor checks, the state's tensors, `on_device`, the cached size query, `_workspace`,
the outputs, the C call — and takes from the module only its gate, its plan and its two C functions with their leading arguments."""
import torch

from . import _lib

_workspaces = {}
_WORKSPACE_CACHE = 16    # (stream, purpose) entries kept PER DEVICE; beyond that the least recently used buffer is released

# Prepared tables (include/cmcd_hip.h: cmcd_bound_forward_prepared): what the forward workspace of (device, buffer address)
# holds, as the key of the call that formed it.  A forward call whose key matches skips the prep launch — evaluation loops on
# fixed parameters (the reference's opt.sample: 30 calls of loss_fn on one params_flat).
# OPT-IN: `with fixed_parameters():` around the loop (or CMCD_PREP_CACHE=1 for the process).  Inside, the key carries the
# parameter tensor's address AND its version counter, and the entry a weak reference to the tensor object: every in-place
# update through torch bumps the counter, and the two places of this package that write parameters through a raw pointer (the
# fused optimiser step, eager and graph-replayed) bump it by hand (torch.autograd.graph.increment_version).  What NO key can
# see is a write that bypasses the counter — `params_flat.data.mul_(...)` (`.data` has a counter of its own), a raw-pointer
# write from other code — which is why the shortcut is not the default: the caller states that the parameters are fixed.
# Never used while a graph is being captured (a captured "no prep" would outlive the parameters).
# (The process-wide flag, PREP_CACHE, stays with its one reader: mcdboundingmachine.bound_forward.)
_prepared = {}
_fixed = __import__("threading").local()


class fixed_parameters:
    """Context of an evaluation loop on unchanged parameters: forward calls inside may reuse the per-parameter tables the
    previous call left in the workspace (cmcd_bound_forward_prepared).  Re-entrant, per host thread."""

    def __enter__(self):
        _fixed.depth = getattr(_fixed, "depth", 0) + 1
        return self

    def __exit__(self, *exc):
        _fixed.depth -= 1
        return False


PREP_CALLS = {"prepared": 0, "full": 0}      # forward calls that skipped / ran the prep launch (tests, bench)


def _workspace(dev_index, device, stream, capturing, nbytes, tag, what=None, retire=False):
    """Scratch buffer of one (device, HIP stream, purpose): calls enqueued on different streams of one device — from
    one host thread or several — never share a workspace, so they may overlap on the GPU (include/cmcd_hip.h: the
    library itself keeps nothing between calls).  Calls on the same stream are ordered and reuse the buffer.
    `dev_index`, `stream`, `capturing` are those of `device` (see _stream).
    `what`: `nbytes` is the answer of a size query, and <= 0 its refusal — NotImplementedError with the library's last error, or
    this text when it left none.  `retire`: the launch rewrites per-parameter tables in the buffer, so whatever claim a forward
    call left on them (see _prepared) goes."""
    if what is not None and nbytes <= 0:
        raise NotImplementedError(_lib.last_error() or what)
    if retire:
        ws = _workspace(dev_index, device, stream, capturing, nbytes, tag)
        _prepared.pop((dev_index, ws.data_ptr()), None)
        return ws
    if capturing:
        # inside torch.cuda.graph(): the buffer must come from (and stay with) the graph's private pool, so it is neither
        # taken from the cache nor put into it — an eager call that later runs on a recycled stream handle never sees it
        return torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
    per_dev = _workspaces.setdefault(dev_index, {})      # one LRU per device: a busy device never evicts another's buffers
    key = (stream, tag)
    ws = per_dev.pop(key, None)              # re-inserted below: the dict is ordered by last use
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
        _prepared.pop((dev_index, ws.data_ptr()), None)      # a fresh buffer holds nobody's tables, whatever lived at its address
    per_dev[key] = ws
    while len(per_dev) > _WORKSPACE_CACHE:         # least recently used first: streams that died, one-off streams
        per_dev.pop(next(iter(per_dev)))
    return ws


def _stream(device):
    """-> (device index, raw handle of the device's current HIP stream, whether that stream is being captured), or None when
    `device` is not the current device: `on_device` then runs the call under torch.cuda.device(device), so that every HIP
    call belongs to the tensor's device (rare; the common case pays no context manager)."""
    dev_index, current = device.index, torch._C._cuda_getDevice()
    if dev_index is None:
        dev_index = current                  # "cuda" is the current device
    elif dev_index != current:
        return None
    return dev_index, torch._C._cuda_getCurrentRawStream(dev_index), torch._C._cuda_isCurrentStreamCapturing()


def on_device(device, body):
    """-> body(dev_index, stream, capturing), run once with what `_stream` answers for `device`: directly when it is the current
    device, otherwise under torch.cuda.device(device) with the stream looked up there.  The body holds the entry point's own C
    call; its size query runs inside it, on the tensor's device.  (A plain function and a tuple: this sits on the host-bound
    path of the smallest configurations, where an object per call was measurable.)"""
    here = _stream(device)
    if here is not None:
        return body(*here)
    with torch.cuda.device(device):
        return body(*_stream(device))


def consts_args(consts):
    """The (pointer, count) pair of the C calls for a target's constants, `Target.consts_on(device)`: a tensor or None."""
    return (None, 0) if consts is None else (consts.data_ptr(), consts.numel())


def _inputs(seeds, params_flat, seedless=False):
    """The tensor checks every entry point makes -> (seeds as a contiguous int32 tensor on params_flat's device, n).
    `seedless` — a chain segment that starts from a state, not from seeds — checks params_flat alone -> (None, 0)."""
    if not params_flat.is_cuda:
        raise RuntimeError("the CMCD hot path runs on a ROCm device only: params_flat is not a device tensor")
    if params_flat.dtype != torch.float32 or not params_flat.is_contiguous():
        raise ValueError("params_flat must be contiguous float32")
    if seedless:
        return None, 0
    device = params_flat.device
    if not isinstance(seeds, torch.Tensor) or seeds.device != device or seeds.dtype != torch.int32 or not seeds.is_contiguous():
        seeds = torch.as_tensor(seeds).to(device=device, dtype=torch.int32).contiguous()
    n = seeds.numel()
    if n < 1:
        raise ValueError("seeds is empty")
    return seeds, n


def check_x(x, n, dim, device):
    """The checks on the target draws `x[n, dim]` of a reverse-time chain, made after `_inputs`."""
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.device != device:
        raise RuntimeError("the CMCD hot path runs on a ROCm device only: x is not a tensor on the device of params_flat")
    if x.dtype != torch.float32 or not x.is_contiguous() or tuple(x.shape) != (n, dim):
        raise ValueError(f"x must be contiguous float32 of shape [n, dim] = [{n}, {dim}]")


def _outputs(n, dim, device):
    """-> (losses[n] f32, z[n, dim] f32, stats[NSTATS] f64), for the library to fill."""
    return (torch.empty(n, dtype=torch.float32, device=device), torch.empty((n, dim), dtype=torch.float32, device=device),
            torch.empty(_lib.NSTATS, dtype=torch.float64, device=device))


def _zero_notrain(grad, unflatten):
    """params_notrain = stop_gradient(params_notrain) (the reference's mcdboundingmachine.py:142, boundingmachine.py:75): only
    the leaves of params_train carry a gradient; they are the leading block of params_flat.  Where that block ends is found
    once per Unflatten."""
    n_train = unflatten.__dict__.get("_n_train", -1)
    if n_train == -1:
        n_train = unflatten._n_train = min((off for path, (off, _) in unflatten.layout.items() if path[0] == 1), default=None)
    if n_train is not None:
        grad[n_train:].zero_()
