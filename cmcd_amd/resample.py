"""The result of a bound evaluation read as a weighted particle system: `losses[N]`, `z[N, dim]`, w_n = exp(-loss_n).

`importance_stats` tells how degenerate the weights behind a ln Z estimate are (effective sample size, largest normalised
weight); `resample` turns `(losses, z)` into approximately target-distributed samples by systematic resampling.  Both are ONE
launch of libcmcd_hip.so (cmcd_resample_systematic, csrc/cmcd_resample.hip) on the current stream: no host round trip, so
they can follow the forward call inside a captured graph.  The reference has no counterpart (it reports W2 on the unweighted
z and stops at logsumexp); the arithmetic is restated in float64 NumPy in tests/test_gpu_resample.py.

Rows are `groups` consecutive groups of N / groups particles — the n_input_dist_seeds x n_samples layout of `utils.sample` —
and every group is weighted, measured and resampled on its own.  No CPU fallback."""
import torch

from . import _lib
from ._call import on_device, _workspace

CHUNK = 1024             # rows a workgroup scans per step (csrc/cmcd_host.h: kResampleChunk); groups longer than this carry a running sum
MAX_GROUP = 1 << 20      # rows per group the library accepts
STATS = ("n_finite", "ln_Z", "ess", "max_weight", "diverged")      # the columns of the library's [groups][5] statistics


def launch(losses, z=None, groups=1, seed=0, index=True, copy=True):
    """cmcd_resample_systematic on device tensors -> (z_resampled | None, index | None, stats[groups, 5] float64).
    `index` / `copy` choose which of the two nullable outputs the library writes (`copy` needs `z`)."""
    if not isinstance(losses, torch.Tensor) or not losses.is_cuda:
        raise RuntimeError("the CMCD hot path runs on a ROCm device only: losses is not a device tensor")
    device = losses.device
    copy = copy and z is not None
    if z is not None and (not isinstance(z, torch.Tensor) or z.device != device):
        raise RuntimeError("the CMCD hot path runs on a ROCm device only: z is not a tensor on the device of losses")
    losses = losses.detach().reshape(-1).to(torch.float32).contiguous()
    n, groups = losses.numel(), int(groups)
    dim = 0
    if z is not None:
        z = z.detach().to(torch.float32).contiguous()
        if n < 1 or z.numel() % n != 0 or z.numel() < n:
            raise ValueError("z must hold one row per loss")
        dim = z.numel() // n

    def run(dev_index, stream, capturing):
        L = _lib.lib()
        nbytes = L.cmcd_resample_workspace_bytes(n, groups)
        # (a size query that answered 0 refused the arguments: the call below refuses them too, with the message)
        ws = _workspace(dev_index, device, stream, capturing, max(nbytes, 16), "resample")
        stats = torch.empty((max(groups, 1), _lib.NSTATS), dtype=torch.float64, device=device)
        out_index = torch.empty(n, dtype=torch.int32, device=device) if index else None
        out_z = torch.empty((n, dim), dtype=torch.float32, device=device) if copy else None
        _lib.check(L.cmcd_resample_systematic(
            losses.data_ptr(), z.data_ptr() if z is not None else None, n, dim, groups, int(seed) & 0xFFFFFFFF, ws.data_ptr(),
            nbytes, out_index.data_ptr() if index else None, out_z.data_ptr() if copy else None, stats.data_ptr(), stream))
        return out_z, out_index, stats

    return on_device(device, run)


def _as_dict(stats):
    return {name: stats[:, i] for i, name in enumerate(STATS)}


def importance_stats(losses, groups=1):
    """-> {"ess", "ln_Z", "max_weight", "n_finite", "diverged"}: float64 device tensors of length `groups` (views of one
    buffer; nothing is copied to the host).  ess = (sum w)^2 / sum w^2 in [1, N / groups]; ln_Z = logsumexp(-loss) - log(N / groups);
    max_weight = the largest normalised weight; a group with a NaN or -inf loss has diverged = 1 and NaN elsewhere."""
    return _as_dict(launch(losses, None, groups, 0, index=False, copy=False)[2])


def resample(losses, z, groups=1, seed=0):
    """Systematic resampling within each group -> (z_resampled[N, dim], index[N] int32, stats as `importance_stats`).
    `index` holds global row numbers, `z_resampled = z[index]`; the one uniform per group is word g of
    jax.random.uniform(PRNGKey(seed), (groups,)) (cmcd_amd/prng.py).  Ancestor j is drawn floor or ceil of
    (N / groups) x its normalised weight times.  Diverged groups and groups without a finite loss come back unchanged."""
    if z is None:
        raise ValueError("resample needs z")
    out_z, index, stats = launch(losses, z, groups, seed)
    return out_z.view(z.shape), index, _as_dict(stats)
