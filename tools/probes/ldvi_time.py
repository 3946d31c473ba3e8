"""Time of the LDVI calls (cmcd_amd.ldvi: prep + ldvi_traj_kernel + finalize; the gradient call adds ldvi_net_grad_kernel,
ldvi_sweep_kernel, ldvi_reduce_kernel and the two tails of cmcd_grad.hip) beside MCD_CAIS_UHA_sn's forward call pinned to its
wave-per-tile kernel (KERNEL_VARIANT = 1: prep + uha_traj_kernel + finalize), same process, same parameters (the tree is the same:
only the mode string differs), at gmm N = 300, K = 8, funnel N = 300, K = 64 and many_gmm N = 2000, K = 256 on the 24-wide
geffner net (emb 20).  Per bridge LDVI does one network evaluation where that kernel does two, the same draws and the same number
of target evaluations, on the same mapping: that kernel at the same shape is the yardstick of the forward call.  The three
callables are alternated window by window; a window is ITERS calls between two device synchronisations on the host clock, so
each figure is the time per call as a user's loop sees it (launches + host work).

    python tools/probes/ldvi_time.py [out.txt]        (the record: profiles/r17_ldvi.txt)
"""
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from cmcd_amd import ldvi, mcdboundingmachine as mcdbm, synthetic  # noqa: E402

WINDOWS = 9
SHAPES = (("gmm_n300_k8", 300, 200, {}),
          ("funnel_n300_k64", 300, 50, dict(init_eps=0.05, init_gamma=4.0)),
          ("many_gmm_n2000_k256_dds", 2000, 20, dict(nn_arch="geffner", emb_dim=20, init_eps=0.2, init_gamma=2.0, init_sigma=15.0)))


def window(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r17_ldvi.txt")
    out = open(path, "w")

    def say(s):
        print(s, flush=True)
        out.write(s + "\n")
        out.flush()

    mcdbm.KERNEL_VARIANT = 1          # MCD_CAIS_UHA_sn's forward call on its wave-per-tile kernel
    say(f"# {torch.cuda.get_device_name(0)}; microseconds per call, median [min .. max] over {WINDOWS} windows; LDVI forward, LDVI "
        "gradient and MCD_CAIS_UHA_sn forward (wave-per-tile) windows alternating")
    for name, n, iters, over in SHAPES:
        b = synthetic.build(name, device="cuda", boundmode="MCD_CAIS_UHA_sn", **over)
        cfg = b["cfg"]
        dim, K, _, spec = b["params_fixed"]
        flat, un, tgt = b["params_flat"], b["unflatten"], b["target"]
        fixed = (dim, K, "MCD_U_a-lp-sn", spec)
        seeds = torch.from_numpy(synthetic.throughput_seeds(n)).cuda()
        fwd = lambda: ldvi.bound_forward(seeds, flat, un, fixed, tgt)                                     # noqa: E731
        grd = lambda: ldvi.grad_and_loss(seeds, flat, un, fixed, tgt)                                     # noqa: E731
        uha = lambda: mcdbm.bound_forward(seeds, flat, un, b["params_fixed"], tgt)                        # noqa: E731
        for f in (fwd, grd, uha):
            window(f, 3)
        tf, tg, tu = [], [], []
        for _ in range(WINDOWS):
            tf.append(window(fwd, iters))
            tg.append(window(grd, iters))
            tu.append(window(uha, iters))
        mf, mu = statistics.median(tf), statistics.median(tu)
        say(f"{cfg['model']} K = {K}, n = {n}, width {2 * dim + spec.emb_dim}, windows of {iters} calls:")
        say(f"  LDVI forward              {mf:9.1f} [{min(tf):9.1f} .. {max(tf):9.1f}]   ratio of medians LDVI forward / 2nd-order "
            f"forward {mf / mu:.2f}; bar (that call's median + its own spread) {mu + max(tu) - min(tu):.1f}: "
            f"{'met' if mf <= mu + max(tu) - min(tu) else 'MISSED'}")
        say(f"  LDVI gradient             {statistics.median(tg):9.1f} [{min(tg):9.1f} .. {max(tg):9.1f}]   ratio of medians LDVI gradient / "
            f"LDVI forward {statistics.median(tg) / mf:.2f}")
        say(f"  MCD_CAIS_UHA_sn forward   {mu:9.1f} [{min(tu):9.1f} .. {max(tu):9.1f}]")
    out.close()


if __name__ == "__main__":
    main()
