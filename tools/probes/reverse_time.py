"""Time of the reverse-time chain (cmcd_amd.mcdboundingmachine.bound_reverse: prep + reverse_traj_kernel + finalize) beside
the forward call pinned to its wave-per-tile kernel (KERNEL_VARIANT = 1: prep + traj_kernel + finalize), same process, same
parameters, at the evaluation shapes 30 x 500 gmm K = 8, 30 x 2000 funnel K = 64 and many_gmm dds K = 256 with 15 000
particles.  The two are alternated window by window; a window is ITERS calls between two device synchronisations on the host
clock, so each figure is the time per call as a user's loop sees it (launches + host work).

    python tools/probes/reverse_time.py [out.txt]
"""
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from cmcd_amd import mcdboundingmachine as mcdbm, synthetic  # noqa: E402
from cmcd_amd.model_handler import exact_target_draws, load_model  # noqa: E402

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

    mcdbm.KERNEL_VARIANT = 1          # the forward call on its wave-per-tile kernel: the reverse call's only form
    say(f"# {torch.cuda.get_device_name(0)}; microseconds per call, median [min .. max] over {WINDOWS} windows, "
        "reverse and forward (wave-per-tile) windows alternating")
    for name, n, iters in (("gmm_n300_k8", 30 * 500, 200), ("funnel_n300_k64", 30 * 2000, 50),
                           ("many_gmm_n2000_k256_dds", 15000, 20)):
        b = synthetic.build(name, device="cuda")
        cfg = b["cfg"]
        seeds = torch.from_numpy(synthetic.throughput_seeds(n)).cuda()
        x = torch.from_numpy(exact_target_draws(cfg["model"], load_model(cfg["model"], None)[2], 3, n, b["params_fixed"][0])).cuda()
        args = (b["params_flat"], b["unflatten"], b["params_fixed"], b["target"])
        kw = dict(eps_schedule=b["eps_schedule"], grad_clipping=b["grad_clipping"])
        rev = lambda: mcdbm.bound_reverse(seeds, x, *args, **kw)      # noqa: E731
        fwd = lambda: mcdbm.bound_forward(seeds, *args, **kw)         # noqa: E731
        for f in (rev, fwd):
            window(f, 5)
        tr, tf = [], []
        for _ in range(WINDOWS):
            tr.append(window(rev, iters))
            tf.append(window(fwd, iters))
        say(f"{cfg['model']} {cfg['nn_arch']} K = {cfg['nbridges']}, n = {n}, windows of {iters} calls:")
        say(f"  reverse  {statistics.median(tr):9.1f} [{min(tr):9.1f} .. {max(tr):9.1f}]")
        say(f"  forward  {statistics.median(tf):9.1f} [{min(tf):9.1f} .. {max(tf):9.1f}]   ratio of medians reverse / forward "
            f"{statistics.median(tr) / statistics.median(tf):.2f}")
    if out:
        out.close()


if __name__ == "__main__":
    main()
