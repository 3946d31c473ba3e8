"""Time of the fused resampling call (cmcd_amd.resample.resample: one launch of cmcd_resample_systematic) beside the same
result composed from stock torch operations (logsumexp, exp, cumsum, searchsorted, index_select), same process, same inputs, at
the evaluation shapes 30 x 500, 30 x 2000 (dim 2) and 30 x 20 (dim 1600).  The two are alternated window by window; a window is
ITERS calls between two device synchronisations on the host clock, so each figure is the time per call as a user's loop sees
it (launches + host work).  Also: one group of 2^18 particles on its single workgroup.

    python tools/probes/resample_time.py [out.txt]
"""
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from cmcd_amd import prng, resample  # noqa: E402

ITERS, WINDOWS = 200, 15


def torch_composition(loss, z, groups, u, ar, base):
    m = loss.numel() // groups
    nl = -loss.view(groups, m).double()
    lse = torch.logsumexp(nl, 1, keepdim=True)
    W = torch.exp(nl - lse)
    ess = 1.0 / (W * W).sum(1)
    C = torch.cumsum(W, 1)
    t = (ar + u) / m
    a = torch.searchsorted(C, t, right=True).clamp_(max=m - 1)
    idx = (a + base).view(-1)
    return z.index_select(0, idx), idx, ess, lse.view(-1) - math.log(m)


def window(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def main():
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else None

    def say(s):
        print(s, flush=True)
        if out:
            out.write(s + "\n")
            out.flush()

    dev = torch.device("cuda", 0)
    say(f"# {torch.cuda.get_device_name(0)}; microseconds per call, median [min .. max] over {WINDOWS} windows of {ITERS} calls, "
        "fused and torch windows alternating")
    gen = torch.Generator().manual_seed(0)
    for groups, m, dim in ((30, 500, 2), (30, 2000, 2), (30, 20, 1600)):
        n = groups * m
        loss = (3.0 * torch.randn(n, generator=gen)).to(dev)
        z = torch.randn(n, dim, generator=gen).to(dev)
        u = torch.from_numpy(prng.uniform(7, (groups,), 0.0, 1.0)).double().to(dev)[:, None]
        ar = torch.arange(m, dtype=torch.float64, device=dev)[None, :]
        base = (torch.arange(groups, device=dev) * m)[:, None]
        fused = lambda: resample.resample(loss, z, groups=groups, seed=7)                    # noqa: E731
        stock = lambda: torch_composition(loss, z, groups, u, ar, base)                      # noqa: E731
        zf, idxf, st = fused()
        zt, idxt, ess, lnz = stock()
        torch.cuda.synchronize()
        say(f"{groups} x {m}, dim {dim}: ancestors that differ between the two {int((idxf.long() != idxt).sum())} of {n}; "
            f"max |ESS diff| {float((st['ess'] - ess).abs().max()):.3g}; max |ln Z diff| {float((st['ln_Z'] - lnz).abs().max()):.3g}")
        for f in (fused, stock):
            window(f, 50)
        tf, tt = [], []
        for _ in range(WINDOWS):
            tf.append(window(fused, ITERS))
            tt.append(window(stock, ITERS))
        say(f"  fused  {statistics.median(tf):8.1f} [{min(tf):8.1f} .. {max(tf):8.1f}]")
        say(f"  torch  {statistics.median(tt):8.1f} [{min(tt):8.1f} .. {max(tt):8.1f}]   ratio of medians torch / fused "
            f"{statistics.median(tt) / statistics.median(tf):.2f}")
        # the same pair replayed from a captured graph: launches only, no host work per call
        graphs = []
        for f in (fused, stock):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                keep = f()
            graphs.append((g, keep))
        for g, _ in graphs:
            window(g.replay, 50)
        gf, gt = [], []
        for _ in range(WINDOWS):
            gf.append(window(graphs[0][0].replay, ITERS))
            gt.append(window(graphs[1][0].replay, ITERS))
        say(f"  fused, graph replay  {statistics.median(gf):8.1f} [{min(gf):8.1f} .. {max(gf):8.1f}]")
        say(f"  torch, graph replay  {statistics.median(gt):8.1f} [{min(gt):8.1f} .. {max(gt):8.1f}]   ratio "
            f"{statistics.median(gt) / statistics.median(gf):.2f}")
    # one group on one workgroup: the case a second-level (multi-block) scan would serve
    for m in (1 << 14, 1 << 18):
        loss = (3.0 * torch.randn(m, generator=gen)).to(dev)
        z = torch.randn(m, 2, generator=gen).to(dev)
        big = lambda: resample.resample(loss, z, groups=1, seed=7)                           # noqa: E731
        window(big, 5)
        tb = [window(big, 20) for _ in range(7)]
        say(f"1 x {m}, dim 2 (single workgroup): fused {statistics.median(tb):8.1f} [{min(tb):8.1f} .. {max(tb):8.1f}]")
    if out:
        out.close()


if __name__ == "__main__":
    main()
