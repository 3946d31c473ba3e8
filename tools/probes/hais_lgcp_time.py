"""Time of the Hamiltonian AIS calls on lgcp (cmcd_amd.hais_lgcp: init + one launch per target evaluation + final + finalize; the
gradient call adds one sweep launch per evaluation and two reductions) beside MCD_ULA's forward call on lgcp, same process, same q,
at K = 128, lfsteps = 1: UHA forward and UHA value + gradient at N = 20 (the BASELINE config 5 shape), UHA forward at N = 600,
MCD_ULA forward at both N.  MCD_ULA is network-free and, like UHA at L = 1, takes K + 1 products with K^-1 per call: its time per
evaluation is the yardstick.  The callables are alternated window by window; a window is ITERS calls between two device
synchronisations on the host clock, so each figure is the time per call as a user's loop sees it (launches + host work).

    python tools/probes/hais_lgcp_time.py [out.txt]            (the record: profiles/r20_hais_lgcp.txt)
    python tools/probes/hais_lgcp_time.py --forward-loop 20    (the N = 20 forward loop alone, for a kernel trace)
"""
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from cmcd_amd import hais_lgcp, mcdboundingmachine as mcdbm, synthetic  # noqa: E402

WINDOWS = 9
K = 128


def window(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def calls(n):
    counts = np.load(os.path.join(ROOT, "tests", "golden", "lgcp_bin_counts.npy"))
    b = synthetic.build("lgcp_n20_k128", device="cuda", boundmode="MCD_ULA", lgcp_counts=counts, nbridges=K, N=n)
    allp = {**b["unflatten"](b["params_flat"])[0], **b["unflatten"](b["params_flat"])[1]}
    vd = {k: v.detach().cpu().clone() for k, v in allp["vd"].items()}
    flat, un, fixed = hais_lgcp.initialize(b["params_fixed"][0], vdparams=vd, nbridges=K, lfsteps=1, eps=float(allp["eps"]), eta=0.5,
                                           trainable=("eta", "eps", "vd", "mgridref_y"), device="cuda")
    seeds = torch.from_numpy(synthetic.throughput_seeds(n)).cuda()
    tgt = b["target"]
    fwd = lambda: hais_lgcp.bound_forward(seeds, flat, un, fixed, tgt)                                     # noqa: E731
    grd = lambda: hais_lgcp.grad_and_loss(seeds, flat, un, fixed, tgt)                                     # noqa: E731
    ula = lambda: mcdbm.bound_forward(seeds, b["params_flat"], b["unflatten"], b["params_fixed"], tgt,      # noqa: E731
                                      eps_schedule=b["eps_schedule"], grad_clipping=b["grad_clipping"])
    return fwd, grd, ula


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--forward-loop":
        fwd, _, _ = calls(20)
        window(fwd, 3)
        print("UHA forward, N = 20: %.1f us per call" % window(fwd, int(sys.argv[2])))
        return
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r20_hais_lgcp.txt")
    out = open(path, "w")

    def say(s):
        print(s, flush=True)
        out.write(s + "\n")
        out.flush()

    say(f"# {torch.cuda.get_device_name(0)}; lgcp (d = 1600), K = {K}, lfsteps = 1: {K + 1} target evaluations per particle in every "
        f"call; microseconds per call, median [min .. max] over {WINDOWS} windows, windows alternating in one process, three warm-up "
        "calls each")
    for n, iters, with_grad in ((20, 20, True), (600, 5, False)):
        fwd, grd, ula = calls(n)
        fns = [("UHA forward", fwd), ("MCD_ULA forward", ula)] + ([("UHA value + gradient", grd)] if with_grad else [])
        for _, f in fns:
            window(f, 3)
        t = {name: [] for name, _ in fns}
        for _ in range(WINDOWS):
            for name, f in fns:
                t[name].append(window(f, iters))
        mu = statistics.median(t["MCD_ULA forward"])
        say(f"N = {n}, windows of {iters} calls:")
        for name, _ in fns:
            v = t[name]
            md = statistics.median(v)
            say(f"  {name:22s} {md:10.1f} [{min(v):10.1f} .. {max(v):10.1f}]   {md / (K + 1):7.2f} per evaluation   "
                f"ratio of medians to MCD_ULA forward {md / mu:.2f}")
    out.close()


if __name__ == "__main__":
    main()
