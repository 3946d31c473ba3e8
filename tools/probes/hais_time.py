"""Time of the Hamiltonian AIS calls (cmcd_amd.hais: hais_traj_kernel + finalize; the gradient call adds hais_grad_kernel and
hais_reduce_kernel) beside MCD_ULA's forward call pinned to its wave-per-tile kernel (KERNEL_VARIANT = 1: prep + traj_kernel +
finalize), same process, same q, same step size, at the evaluation shapes 30 x 500 gmm K = 8, 30 x 2000 funnel K = 64 and
many_gmm K = 256 with 15 000 particles, lfsteps = 1.  At L = 1 the chain does one target evaluation and one Threefry stage per
bridge, which is what MCD_ULA does: that kernel at the same shape is the yardstick.  The three callables are alternated window
by window; a window is ITERS calls between two device synchronisations on the host clock, so each figure is the time per call
as a user's loop sees it (launches + host work).

    python tools/probes/hais_time.py [out.txt]        (the record: profiles/r13_hais.txt)
"""
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from cmcd_amd import hais, mcdboundingmachine as mcdbm, synthetic  # noqa: E402

WINDOWS = 9


def window(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r13_hais.txt")
    out = open(path, "w")

    def say(s):
        print(s, flush=True)
        out.write(s + "\n")
        out.flush()

    mcdbm.KERNEL_VARIANT = 1          # MCD_ULA's forward call on its wave-per-tile kernel
    say(f"# {torch.cuda.get_device_name(0)}; microseconds per call, median [min .. max] over {WINDOWS} windows; UHA forward, UHA "
        "gradient and MCD_ULA forward (wave-per-tile) windows alternating; lfsteps = 1")
    for name, n, iters in (("gmm_n300_k8", 30 * 500, 100), ("funnel_n300_k64", 30 * 2000, 30),
                           ("many_gmm_n2000_k256_dds", 15000, 10)):
        b = synthetic.build(name, device="cuda", boundmode="MCD_ULA")
        cfg = b["cfg"]
        K = cfg["nbridges"]
        allp = {**b["unflatten"](b["params_flat"])[0], **b["unflatten"](b["params_flat"])[1]}
        vd = {k: v.detach().cpu().clone() for k, v in allp["vd"].items()}
        dim = b["params_fixed"][0]
        flat, un, fixed = hais.initialize(dim, vdparams=vd, nbridges=K, lfsteps=1, eps=float(allp["eps"]), eta=0.5,
                                          trainable=("eta", "eps", "vd", "mgridref_y"), device="cuda")
        seeds = torch.from_numpy(synthetic.throughput_seeds(n)).cuda()
        tgt = b["target"]
        fwd = lambda: hais.bound_forward(seeds, flat, un, fixed, tgt)                                     # noqa: E731
        grd = lambda: hais.grad_and_loss(seeds, flat, un, fixed, tgt)                                     # noqa: E731
        ula = lambda: mcdbm.bound_forward(seeds, b["params_flat"], b["unflatten"], b["params_fixed"], tgt,  # noqa: E731
                                          eps_schedule=b["eps_schedule"], grad_clipping=b["grad_clipping"])
        for f in (fwd, grd, ula):
            window(f, 3)
        tf, tg, tu = [], [], []
        for _ in range(WINDOWS):
            tf.append(window(fwd, iters))
            tg.append(window(grd, iters))
            tu.append(window(ula, iters))
        mu = statistics.median(tu)
        say(f"{cfg['model']} K = {K}, n = {n}, windows of {iters} calls:")
        say(f"  UHA forward      {statistics.median(tf):9.1f} [{min(tf):9.1f} .. {max(tf):9.1f}]   ratio of medians UHA forward / MCD_ULA "
            f"forward {statistics.median(tf) / mu:.2f}")
        say(f"  UHA gradient     {statistics.median(tg):9.1f} [{min(tg):9.1f} .. {max(tg):9.1f}]   ratio of medians UHA gradient / MCD_ULA "
            f"forward {statistics.median(tg) / mu:.2f}")
        say(f"  MCD_ULA forward  {mu:9.1f} [{min(tu):9.1f} .. {max(tu):9.1f}]")
    out.close()


if __name__ == "__main__":
    main()
