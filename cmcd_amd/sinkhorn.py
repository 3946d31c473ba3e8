"""Batched Sinkhorn W2 between equal-size point clouds on the device: the evaluation's third metric
(/root/reference/src/utils.py:207-216,251-282) for all seed groups at once.

`w2_batched` solves G independent entropic OT problems with the arithmetic of `utils.W2_distance` — float64, cost matrix
divided by its maximum, Sinkhorn-Knopp with a marginal check every 10 iterations — in libcmcd_hip.so
(cmcd_sinkhorn_setup / _iterate / _cost, csrc/cmcd_sinkhorn.hip): one launch per iteration carries every problem, finished
problems drop out on a per-problem word, and the host looks at those words only every `poll_every` iterations.  Every sum has a
fixed order, so a problem's result does not depend on the batch it is solved in.  The arithmetic is restated in
tests/test_gpu_sinkhorn.py.  No CPU fallback."""
import torch

from . import _lib
from ._call import on_device, _workspace

ROWS = 64                # rows of K per workgroup (csrc/cmcd_host.h: kSinkhornRows)
MAX_N = 8192             # points per cloud the library accepts
MAX_GROUPS = 65535       # problems per library call; larger batches are split here
FIELDS = ("cost", "iterations", "err", "status")       # the columns of the library's [G][4] record
CONVERGED, CAPPED, UNSOLVABLE = 0, 1, 2


def _f64(t, device, name, shape=None):
    if not isinstance(t, torch.Tensor) or not t.is_cuda or (device is not None and t.device != device):
        raise RuntimeError(f"the CMCD hot path runs on a ROCm device only: {name} is not a device tensor"
                           + ("" if device is None else " on the device of x"))
    t = t.detach().to(torch.float64).contiguous()
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must have shape {tuple(shape)}, got {tuple(t.shape)}")
    return t


def w2_batched(x, y, a=None, b=None, reg=0.01, num_iter_max=10000, stop_thr=1e-16, poll_every=500,
               max_workspace_bytes=2 << 30):
    """x, y: [G, n, d] device tensors; a, b: [G, n] weights or None (uniform 1 / n) -> {"cost", "iterations", "err", "status"}:
    float64 device tensors of length G (views of one buffer).  status 0 = converged (err < stop_thr at a check), 1 = stopped at
    num_iter_max, 2 = a non-finite coordinate or weight, or all points equal (cost NaN).

    `poll_every` iterations are enqueued between two looks at the problems' done words (one small device->host copy);
    `poll_every=0` never looks and enqueues all num_iter_max launches — nothing synchronises, the form for graph capture.
    A batch whose workspace would exceed `max_workspace_bytes` is solved in slices of the groups, with identical results."""
    x = _f64(x, None, "x")
    if x.dim() != 3:
        raise ValueError("x must have shape [G, n, d]")
    device = x.device
    y = _f64(y, device, "y", x.shape)
    G, n, dim = x.shape
    a = None if a is None else _f64(a, device, "a", (G, n))
    b = None if b is None else _f64(b, device, "b", (G, n))
    num_iter_max, poll_every = int(num_iter_max), int(poll_every)
    if G < 1:
        raise ValueError("no problems")

    def solve(dev_index, stream, capturing):
        if capturing and poll_every:
            raise RuntimeError("w2_batched under graph capture needs poll_every=0 (polling reads the done words back)")
        L = _lib.lib()
        per = L.cmcd_sinkhorn_workspace_bytes(n, dim, 1)
        # (a size query that answered 0 refused the shape: the setup call below refuses it too, with the message)
        chunk = min(G, MAX_GROUPS, max(1, int(max_workspace_bytes) // per)) if per > 0 else min(G, MAX_GROUPS)
        out = torch.empty((G, 4), dtype=torch.float64, device=device)
        flags = torch.empty(chunk, dtype=torch.int32, device=device) if poll_every else None
        for g0 in range(0, G, chunk):
            g = min(chunk, G - g0)
            nbytes = L.cmcd_sinkhorn_workspace_bytes(n, dim, g)
            ws = _workspace(dev_index, device, stream, capturing, max(nbytes, 16), "sinkhorn")
            xs, ys = x[g0:g0 + g], y[g0:g0 + g]
            _lib.check(L.cmcd_sinkhorn_setup(
                xs.data_ptr(), ys.data_ptr(), a[g0:g0 + g].data_ptr() if a is not None else None,
                b[g0:g0 + g].data_ptr() if b is not None else None, n, dim, g, float(reg), ws.data_ptr(), nbytes, stream))
            it = 0
            while it < num_iter_max:
                count = min(poll_every, num_iter_max - it) if poll_every else num_iter_max - it
                _lib.check(L.cmcd_sinkhorn_iterate(n, dim, g, it, count, num_iter_max, float(stop_thr), ws.data_ptr(), nbytes,
                                                   flags.data_ptr() if poll_every else None, stream))
                it += count
                if poll_every and it < num_iter_max and bool(flags[:g].all()):
                    break
            _lib.check(L.cmcd_sinkhorn_cost(xs.data_ptr(), ys.data_ptr(), n, dim, g, ws.data_ptr(), nbytes,
                                            out[g0:g0 + g].data_ptr(), None, stream))
        return {name: out[:, i] for i, name in enumerate(FIELDS)}

    return on_device(device, solve)
