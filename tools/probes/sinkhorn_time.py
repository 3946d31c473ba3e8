"""Time of the batched Sinkhorn W2 (cmcd_amd.sinkhorn.w2_batched: one launch per iteration for all problems) beside the loop it
replaces (utils.W2_distance per problem, float64 torch on the device, as utils.calculate_W2_distances(batched=False) runs it),
same process, same inputs: the 2 x 30 problems of one evaluation (cloud -> target, target -> other target) at 30 x 500 gmm
draws (d = 2), 30 x 500 funnel draws (d = 10) and 30 x 2000 gmm draws (d = 2).  The two are alternated window by window; a window
is ONE solve of all 60 problems between two device synchronisations on the host clock (the loop synchronises by itself every
10 iterations), so each figure is the time of the metric as main.py sees it.  The iteration counts of the loop come from one
untimed copy of W2_distance's loop that counts (W2_distance returns the cost alone).

    python tools/probes/sinkhorn_time.py [out.txt]
"""
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from cmcd_amd import sinkhorn, utils  # noqa: E402

WINDOWS_BATCHED, WINDOWS_LOOP = 7, 3


def gmm_draws(rng, groups, n, d):
    means = rng.normal(size=(6, d)) * 4.0
    return (means[rng.integers(0, 6, (groups, n))] + 0.7 * rng.normal(size=(groups, n, d))).astype(np.float32)


def funnel_draws(rng, groups, n, d, s=3.0):
    x0 = s * rng.normal(size=(groups, n, 1))
    return np.concatenate([x0, np.exp(x0 / 2) * rng.normal(size=(groups, n, d - 1))], axis=2).astype(np.float32)


def counting_loop(x, y, reg=0.01, num_iter_max=10000, stop_thr=1e-16):
    """utils.W2_distance with the iteration count"""
    n = x.shape[0]
    a = torch.full((n,), 1.0 / n, dtype=torch.float64, device=x.device)
    b = a.clone()
    M = torch.cdist(x, y) ** 2
    M = M / M.max()
    K = torch.exp(-M / reg)
    u, v = torch.ones_like(a) / n, torch.ones_like(b) / n
    done = 0
    for it in range(num_iter_max):
        v = b / (K.t() @ u)
        u = a / (K @ v)
        done = it + 1
        if it % 10 == 0 and float(torch.linalg.norm(v * (K.t() @ u) - b) ** 2) < stop_thr:
            break
    return done


def window(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else None

    def say(s):
        print(s, flush=True)
        if out:
            out.write(s + "\n")
            out.flush()

    dev = torch.device("cuda", 0)
    say(f"# {torch.cuda.get_device_name(0)}; milliseconds per solve of 60 problems, median [min .. max] over {WINDOWS_BATCHED} "
        f"(batched) / {WINDOWS_LOOP} (loop) windows, alternating; host clock around one solve, device idle before and after")
    rng = np.random.default_rng(0)
    shapes = (("30 x 500 gmm draws, d = 2", gmm_draws, 30, 500, 2), ("30 x 500 funnel draws, d = 10", funnel_draws, 30, 500, 10),
              ("30 x 2000 gmm draws, d = 2", gmm_draws, 30, 2000, 2))
    for name, draw, groups, n, d in shapes:
        cloud = draw(rng, groups, n, d) * np.float32(0.9)          # a sampler that is a little too narrow
        tgt, other = draw(rng, groups, n, d), draw(rng, groups, n, d)
        x = torch.from_numpy(np.concatenate([cloud, tgt])).double().to(dev)
        y = torch.from_numpy(np.concatenate([tgt, other])).double().to(dev)
        batched = lambda: sinkhorn.w2_batched(x, y)                                              # noqa: E731
        loop = lambda: [utils.W2_distance(x[g], y[g]) for g in range(2 * groups)]              # noqa: E731
        _, res = window(batched)                                    # warm-up of both sides, and the agreement
        _, costs = window(loop)
        diff = float((res["cost"].cpu() - torch.tensor(costs, dtype=torch.float64)).abs().max())
        its = res["iterations"].cpu().numpy().astype(int)
        its_loop = np.array([counting_loop(x[g], y[g]) for g in range(2 * groups)])
        say(f"{name}: 60 problems; iterations batched min {its.min()} median {int(np.median(its))} max {its.max()} (at the cap: "
            f"{int((res['status'].cpu() == 1).sum())}), loop min {its_loop.min()} median {int(np.median(its_loop))} max {its_loop.max()}; "
            f"problems whose counts differ {int((its != its_loop).sum())}; max |cost diff| {diff:.3g} -> all within 1e-10: {diff <= 1e-10}")
        tb, tl = [], []
        for w in range(max(WINDOWS_BATCHED, WINDOWS_LOOP)):
            if w < WINDOWS_BATCHED:
                tb.append(window(batched)[0])
            if w < WINDOWS_LOOP:
                tl.append(window(loop)[0])
        say(f"  batched {statistics.median(tb):10.1f} [{min(tb):10.1f} .. {max(tb):10.1f}]   "
            f"({statistics.median(tb) * 1e3 / max(int(its.max()), 1):.1f} us per iteration launch at the longest problem's count)")
        say(f"  loop    {statistics.median(tl):10.1f} [{min(tl):10.1f} .. {max(tl):10.1f}]   ratio of medians loop / batched "
            f"{statistics.median(tl) / statistics.median(tb):.1f}")
        # the unpolled form enqueues every launch up to the cap: what the per-launch cost is when nothing is left to do
        t0 = [window(lambda: sinkhorn.w2_batched(x, y, poll_every=0))[0] for _ in range(3)]
        say(f"  batched, poll_every=0 (10 001 launches whatever the problems need) {statistics.median(t0):10.1f} "
            f"[{min(t0):10.1f} .. {max(t0):10.1f}]")
    if out:
        out.close()


if __name__ == "__main__":
    main()
