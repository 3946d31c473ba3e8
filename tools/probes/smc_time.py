"""Time of the chain segments (cmcd_amd.smc.segment: prep + segment_traj_kernel + finalize) and of the SMC driver beside the
forward call pinned to its wave-per-tile kernel (KERNEL_VARIANT = 1: prep + traj_kernel + finalize), same process, same
parameters, at the evaluation shapes 30 x 500 gmm K = 8, 30 x 2000 funnel K = 64 and many_gmm dds K = 256 with 15 000
particles.  Three callables are alternated window by window: the single segment [0, K), an eight-cut `smc_bound` (seven cuts at
K = 8, where a cut sits at every bridge) in 30 groups with ess_threshold = 0.5, and the forward call.  A window is ITERS calls
between two device synchronisations on the host clock, so each figure is the time per call as a user's loop sees it (launches +
host work).

    python tools/probes/smc_time.py [out.txt]        (the record: profiles/r11_smc.txt)
"""
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from cmcd_amd import mcdboundingmachine as mcdbm, smc, synthetic  # noqa: E402

WINDOWS = 9


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

    mcdbm.KERNEL_VARIANT = 1          # the forward call on its wave-per-tile kernel: the segment call's only form
    say(f"# {torch.cuda.get_device_name(0)}; microseconds per call, median [min .. max] over {WINDOWS} windows, "
        "segment [0, K), smc_bound and forward (wave-per-tile) windows alternating")
    for name, n, iters in (("gmm_n300_k8", 30 * 500, 100), ("funnel_n300_k64", 30 * 2000, 30),
                           ("many_gmm_n2000_k256_dds", 15000, 10)):
        b = synthetic.build(name, device="cuda")
        cfg = b["cfg"]
        K = cfg["nbridges"]
        seeds = torch.from_numpy(synthetic.throughput_seeds(n)).cuda()
        args = (b["params_flat"], b["unflatten"], b["params_fixed"], b["target"])
        kw = dict(eps_schedule=b["eps_schedule"], grad_clipping=b["grad_clipping"])
        cuts = smc.default_cuts(K)
        seg = lambda: smc.segment(seeds, 0, K, *args, **kw)                                              # noqa: E731
        drv = lambda: smc.smc_bound(seeds, *args, **kw, groups=30, cuts=cuts, ess_threshold=0.5)         # noqa: E731
        fwd = lambda: mcdbm.bound_forward(seeds, *args, **kw)                                            # noqa: E731
        for f in (seg, drv, fwd):
            window(f, 3)
        ts, td, tf = [], [], []
        for _ in range(WINDOWS):
            ts.append(window(seg, iters))
            td.append(window(drv, max(1, iters // 4)))
            tf.append(window(fwd, iters))
        events = int(drv()["resampled"].sum())
        mf = statistics.median(tf)
        say(f"{cfg['model']} {cfg['nn_arch']} K = {K}, n = {n}, windows of {iters} calls ({max(1, iters // 4)} for smc_bound), "
            f"{len(cuts)} cuts, {events} resampling events of {len(cuts) * 30}:")
        say(f"  segment [0, K)  {statistics.median(ts):9.1f} [{min(ts):9.1f} .. {max(ts):9.1f}]   ratio of medians segment / forward "
            f"{statistics.median(ts) / mf:.2f}")
        say(f"  smc_bound       {statistics.median(td):9.1f} [{min(td):9.1f} .. {max(td):9.1f}]   ratio of medians smc_bound / forward "
            f"{statistics.median(td) / mf:.2f}")
        say(f"  forward         {mf:9.1f} [{min(tf):9.1f} .. {max(tf):9.1f}]")
    if out:
        out.close()


if __name__ == "__main__":
    main()
