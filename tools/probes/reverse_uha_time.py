"""Time of the reverse-time chain of 2nd-order CMCD (cmcd_amd.reverse_uha.bound_reverse: prep + reverse_uha_kernel + finalize)
beside the MCD_CAIS_UHA_sn forward call pinned to its wave-per-tile kernel (KERNEL_VARIANT = 1: prep + uha_traj_kernel + finalize),
same process, same parameters, at gmm N = 300 K = 8, funnel N = 300 K = 64 and many_gmm (dds) N = 2000 K = 256.  The reverse kernel
does the forward kernel's per-bridge work (K + 1 target evaluations, 2 K network evaluations, one Threefry stage and one density
pair); per call it adds one d-wide draw, the x read and the rho_0 store.  x: exact target draws (generator seed 3).

Device events around windows of ITERS calls, the two callables alternating window by window; per process the median over the
windows; the record holds the median over PROCESSES fresh processes and every process's figure (the spread between them is the
lease-to-lease spread a ratio has to be read against).  many_gmm runs with init_eps = 0.05 (eta = gamma eps < 1: a chain that
stays finite).

    python tools/probes/reverse_uha_time.py [out.txt]        (the record: profiles/r19_reverse_uha.txt, timing section)
    python tools/probes/reverse_uha_time.py --child          (one process: prints one line per shape)
"""
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

WINDOWS, PROCESSES = 9, 3
SHAPES = (("gmm_n300_k8", {}, 300, 200), ("funnel_n300_k64", {}, 300, 50), ("many_gmm_n2000_k256_dds", dict(init_eps=0.05), 2000, 20))


def child():
    import torch
    from cmcd_amd import mcdboundingmachine as mcdbm, reverse_uha, synthetic
    from cmcd_amd.model_handler import exact_target_draws, load_model

    def window(fn, iters):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for _ in range(iters):
            fn()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) / iters * 1e3      # microseconds per call

    mcdbm.KERNEL_VARIANT = 1
    for name, over, n, iters in SHAPES:
        b = synthetic.build(name, device="cuda", boundmode="MCD_CAIS_UHA_sn", **over)
        K = b["cfg"]["nbridges"]
        seeds = torch.from_numpy(synthetic.throughput_seeds(n)).cuda()
        args = (b["params_flat"], b["unflatten"], b["params_fixed"], b["target"])
        sampler = load_model(b["cfg"]["model"], None)[2]
        x = torch.from_numpy(exact_target_draws(b["cfg"]["model"], sampler, 3, n, b["params_fixed"][0])).cuda()
        rev = lambda: reverse_uha.bound_reverse(seeds, x, *args)      # noqa: E731
        fwd = lambda: mcdbm.bound_forward(seeds, *args)               # noqa: E731
        for f in (rev, fwd):
            window(f, 5)
        ts, tf = [], []
        for _ in range(WINDOWS):
            ts.append(window(rev, iters))
            tf.append(window(fwd, iters))
        print("RESULT %s %d %d %.3f %.3f %.3f %.3f %.3f %.3f" % (name, n, K, statistics.median(ts), min(ts), max(ts),
                                                              statistics.median(tf), min(tf), max(tf)), flush=True)


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
                rows.setdefault((f[1], int(f[2]), int(f[3])), []).append([float(x) for x in f[4:]])
    say(f"# microseconds per call from device events; per process the median [min .. max] over {WINDOWS} alternating windows; "
        f"{PROCESSES} processes")
    for (name, n, K), procs in rows.items():
        rev, fwd = [p[0] for p in procs], [p[3] for p in procs]
        ms, mf = statistics.median(rev), statistics.median(fwd)
        say(f"{name} MCD_CAIS_UHA_sn n = {n} K = {K}:")
        say("  reverse chain             median of processes %9.1f   per process %s" % (ms, "  ".join("%.1f [%.1f .. %.1f]" % tuple(p[:3]) for p in procs)))
        say("  forward (wave per tile)   median of processes %9.1f   per process %s" % (mf, "  ".join("%.1f [%.1f .. %.1f]" % tuple(p[3:]) for p in procs)))
        say("  ratio of medians reverse / forward %.3f   per process %s   forward's spread between processes %.1f %%" % (
            ms / mf, "  ".join("%.3f" % (p[0] / p[3]) for p in procs), 100.0 * (max(fwd) - min(fwd)) / mf))
    if out:
        out.close()


if __name__ == "__main__":
    child() if "--child" in sys.argv else main()
