"""Time of the whole-chain segment of LDVI (cmcd_amd.smc_ldvi.segment(seeds, 0, K): prep + segment_ldvi_kernel + finalize) and of UHA
(cmcd_amd.smc_hais.segment(seeds, 0, K): segment_hais_kernel + finalize) beside the forward call of the same mode (ldvi.bound_forward:
prep + ldvi_traj_kernel + finalize; hais.bound_forward: hais_traj_kernel + finalize), same process, same parameters, at gmm N = 300
K = 8, funnel N = 300 K = 64 and many_gmm N = 2000 K = 256.  UHA runs at lfsteps = 1.  Per bridge the segment kernels do the forward
kernels' work; per call they additionally store rho, wpath, lg and the key of every particle.

Device events around windows of ITERS calls, the two callables alternating window by window; per process the median over the
windows; the record holds the median over PROCESSES fresh processes and every process's figure (the spread between them is the
lease-to-lease spread a ratio has to be read against).  A third line gives the HOST time per call — the wall clock over a window
whose calls are enqueued and not waited for: where it equals the device-event figure the call is bound by the host, and a ratio
there compares two Python call paths, not two kernels.  Step sizes are those of tools/probes/reverse_ldvi_hais_time.py, chosen so
that the chains stay finite (LDVI: gamma eps < 1).

    python tools/probes/segment_ldvi_hais_time.py [out.txt]        (the record: profiles/r22_segment_ldvi_hais.txt, timing section)
    python tools/probes/segment_ldvi_hais_time.py --child          (one process: prints one line per mode and shape)
"""
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

WINDOWS, PROCESSES = 9, 3
# (configuration, LDVI overrides, UHA (eps, sigma of q), n, calls per window)
SHAPES = (("gmm_n300_k8", {}, (0.05, 2.0), 300, 200),
          ("funnel_n300_k64", dict(init_eps=0.01, init_gamma=4.0), (0.02, 1.0), 300, 50),
          ("many_gmm_n2000_k256_dds", dict(nn_arch="geffner", emb_dim=20, init_eps=0.05, init_gamma=2.0), (0.05, 15.0), 2000, 20))


def child():
    import torch
    from cmcd_amd import hais, ldvi, smc_hais, smc_ldvi, synthetic
    from cmcd_amd import variationaldist as vd

    def window(fn, iters):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for _ in range(iters):
            fn()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) / iters * 1e3      # microseconds per call

    def host(fn, iters):
        """microseconds of host time per call: the wall clock over `iters` calls that are enqueued and not waited for"""
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        return (t1 - t0) / iters * 1e6

    def measure(tag, name, n, K, seg, fwd, iters):
        for f in (seg, fwd):
            window(f, 5)
        ts, tf = [], []
        for _ in range(WINDOWS):
            ts.append(window(seg, iters))
            tf.append(window(fwd, iters))
        hs, hf = (statistics.median(host(f, iters) for _ in range(3)) for f in (seg, fwd))
        print("RESULT %s %s %d %d %.3f %.3f %.3f %.3f %.3f %.3f %.3f %.3f" % (tag, name, n, K, statistics.median(ts), min(ts), max(ts),
                                                                           statistics.median(tf), min(tf), max(tf), hs, hf), flush=True)

    for name, over, (h_eps, h_sigma), n, iters in SHAPES:
        b = synthetic.build(name, device="cuda", boundmode="MCD_CAIS_UHA_sn", **over)      # the tree LDVI shares with 2nd-order CMCD
        dim, K, _, spec = b["params_fixed"]
        target = b["target"]
        seeds = torch.from_numpy(synthetic.throughput_seeds(n)).cuda()
        la = (b["params_flat"], b["unflatten"], (dim, K, "MCD_U_a-lp-sn", spec), target)
        measure("LDVI", name, n, K, lambda: smc_ldvi.segment(seeds, 0, K, *la), lambda: ldvi.bound_forward(seeds, *la), iters)
        flat, un, fixed = hais.initialize(dim=dim, nbridges=K, lfsteps=1, eps=h_eps, eta=0.5, vdparams=vd.initialize(dim, init_sigma=h_sigma),
                                          trainable=("eta", "eps", "vd", "mgridref_y"), device="cuda")
        ha = (flat, un, fixed, target)
        measure("UHA", name, n, K, lambda: smc_hais.segment(seeds, 0, K, *ha), lambda: hais.bound_forward(seeds, *ha), iters)


def main():
    out = open(sys.argv[1], "w") if len(sys.argv) > 1 else None

    def say(s):
        print(s, flush=True)
        if out:
            out.write(s + "\n")
            out.flush()

    rows = {}
    for _ in range(PROCESSES):      # fresh processes, one after the other; a process that fails ends the probe
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], capture_output=True, text=True, timeout=240)
        if r.returncode != 0:
            say("child failed with %d:\n%s" % (r.returncode, r.stderr[-2000:]))
            sys.exit(1)
        for line in r.stdout.splitlines():
            if line.startswith("RESULT "):
                f = line.split()
                rows.setdefault((f[1], f[2], int(f[3]), int(f[4])), []).append([float(x) for x in f[5:]])
    say(f"# microseconds per call from device events; per process the median [min .. max] over {WINDOWS} alternating windows; "
        f"{PROCESSES} processes")
    for (tag, name, n, K), procs in rows.items():
        seg, fwd = [p[0] for p in procs], [p[3] for p in procs]
        ms, mf = statistics.median(seg), statistics.median(fwd)
        say(f"{tag} {name} n = {n} K = {K}:")
        say("  whole segment   median of processes %9.1f   per process %s" % (ms, "  ".join("%.1f [%.1f .. %.1f]" % tuple(p[:3]) for p in procs)))
        say("  forward call    median of processes %9.1f   per process %s" % (mf, "  ".join("%.1f [%.1f .. %.1f]" % tuple(p[3:6]) for p in procs)))
        say("  host time per call (enqueued, not waited for): segment %s   forward %s" % (
            "  ".join("%.1f" % p[6] for p in procs), "  ".join("%.1f" % p[7] for p in procs)))
        say("  ratio of medians segment / forward %.3f   per process %s   forward's spread between processes %.1f %%" % (
            ms / mf, "  ".join("%.3f" % (p[0] / p[3]) for p in procs), 100.0 * (max(fwd) - min(fwd)) / mf))
    if out:
        out.close()


if __name__ == "__main__":
    child() if "--child" in sys.argv else main()
