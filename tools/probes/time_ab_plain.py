"""Timing A/B of two builds of libcmcd_hip.so over the calls whose kernels take pieces from cmcd_tile.h (CHANGELOG round 16): the
Hamiltonian AIS forward and gradient calls at the three shapes of hais_time.py, the VarGrad value-and-gradient call
(compute_log_var_grad) at the training shape many_gmm_var_n16000_k256 (by the measured rule, which takes work items there, and
pinned to whole chains, the instances that changed) and on gmm K = 8 with 15 000 particles pinned to whole chains, and the
mean-field call on many_gmm with 15 000 particles.  Each library lives in PROCS child processes for the whole run
(CMCD_LIB_PATH); this process asks the children for one window at a time, A1, B1, A2, B2, ..., WINDOWS times per child and call,
so both libraries see the same minutes of the machine.  A window is `iters` calls between two device synchronisations on the
host clock, sized to last about WINDOW_S.  Two processes per library because most of these calls are bound by the host's launch
path, and that may differ from one process to the next by more than a process's windows differ among themselves; a library's
windows are those of both its processes, and the medians of the processes are printed one by one beside them.
Verdict per call: B's median is not above A's median plus A's own max - min — the spread a rebuild of A would show.
A child that does not answer within ANSWER_S, or ends, ends the run: every child is killed and nothing more is started.
    python tools/probes/time_ab_plain.py <previous libcmcd_hip.so> cmcd_amd/libcmcd_hip.so [out.txt]"""
import os
import select
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
WINDOWS = 9
PROCS = 2
WINDOW_S = 0.25
ANSWER_S = 120      # set-up, or one window with its warm-up, takes seconds
HAIS = (("gmm_n300_k8", 30 * 500), ("funnel_n300_k64", 30 * 2000), ("many_gmm_n2000_k256_dds", 15000))
CALLS = [f"hais {kind} {name} n={n}" for name, n in HAIS for kind in ("forward", "gradient")] + \
        ["vargrad many_gmm_var_n16000_k256 n=16000 measured rule", "vargrad many_gmm_var_n16000_k256 n=16000 whole chains",
         "vargrad gmm_n300_k8 n=15000 whole chains", "mfvi gradient many_gmm n=15000"]


def child():
    sys.path.insert(0, ROOT)
    import torch
    from cmcd_amd import boundingmachine as bm, hais, mcdboundingmachine as mcdbm, synthetic
    fns = {}
    for name, n in HAIS:      # hais_time.py's set-up
        b = synthetic.build(name, device="cuda", boundmode="MCD_ULA")
        allp = {**b["unflatten"](b["params_flat"])[0], **b["unflatten"](b["params_flat"])[1]}
        vd = {k: v.detach().cpu().clone() for k, v in allp["vd"].items()}
        flat, un, fixed = hais.initialize(b["params_fixed"][0], vdparams=vd, nbridges=b["cfg"]["nbridges"], lfsteps=1,
                                          eps=float(allp["eps"]), eta=0.5, trainable=("eta", "eps", "vd", "mgridref_y"), device="cuda")
        seeds = torch.from_numpy(synthetic.throughput_seeds(n)).cuda()
        fns[f"hais forward {name} n={n}"] = lambda a=(seeds, flat, un, fixed, b["target"]): hais.bound_forward(*a)
        fns[f"hais gradient {name} n={n}"] = lambda a=(seeds, flat, un, fixed, b["target"]): hais.grad_and_loss(*a)
        if name.startswith("many_gmm"):
            mf, mun, mfixed = bm.initialize(2, vdparams=vd, trainable=("vd",), device="cuda")
            fns[f"mfvi gradient many_gmm n={n}"] = lambda a=(seeds, mf, mun, mfixed, b["target"]): bm.grad_and_loss(*a)

    def vargrad(name, n, item, **over):
        b = synthetic.build(name, device="cuda", **over)
        seeds = torch.from_numpy(synthetic.throughput_seeds(n)).cuda()
        args = (seeds, b["params_flat"], b["unflatten"], b["params_fixed"], b["target"])
        kw = dict(eps_schedule=b["eps_schedule"], grad_clipping=b["grad_clipping"])

        def call():
            os.environ.pop("CMCD_GRAD_ITEM", None)
            if item is not None:
                os.environ["CMCD_GRAD_ITEM"] = item
            return mcdbm.compute_log_var_grad(*args, **kw)
        return call
    fns["vargrad many_gmm_var_n16000_k256 n=16000 measured rule"] = vargrad("many_gmm_var_n16000_k256", 16000, None)
    fns["vargrad many_gmm_var_n16000_k256 n=16000 whole chains"] = vargrad("many_gmm_var_n16000_k256", 16000, "0")
    fns["vargrad gmm_n300_k8 n=15000 whole chains"] = vargrad("gmm_n300_k8", 15000, "0", boundmode="MCD_CAIS_var_sn")
    assert set(fns) == set(CALLS)

    def window(fn, iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / iters * 1e6

    print("ready " + torch.cuda.get_device_name(0), flush=True)
    for line in sys.stdin:           # "<iters> <call>": iters = 0 warms up and answers the time of one call
        iters, call = line.rstrip("\n").split(" ", 1)
        if int(iters) == 0:
            window(fns[call], 3)
            print(window(fns[call], 3), flush=True)
        else:
            print(window(fns[call], int(iters)), flush=True)


def main():
    libs = [os.path.abspath(p) for p in sys.argv[1:3]]
    out = open(sys.argv[3], "w") if len(sys.argv) > 3 else None

    def say(s):
        print(s, flush=True)
        if out:
            out.write(s + "\n")
            out.flush()

    kids = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child"], env=dict(os.environ, CMCD_LIB_PATH=lib),
                             stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, bufsize=1) for _ in range(PROCS) for lib in libs]

    def answer(kid):
        if not select.select([kid.stdout], [], [], ANSWER_S)[0]:
            raise SystemExit("a child process did not answer within %d s" % ANSWER_S)
        line = kid.stdout.readline()
        if not line:
            raise SystemExit("a child process ended (exit status %s)" % kid.wait())
        return line.strip()

    def ask(kid, iters, call):
        kid.stdin.write(f"{iters} {call}\n")
        kid.stdin.flush()
        return float(answer(kid))

    try:
        names = [answer(kid) for kid in kids]
        if not all(n.startswith("ready") for n in names):
            raise SystemExit("a child process did not start: %r" % (names,))
        say(f"# {names[0][6:]}; microseconds per call, median [min .. max] over {PROCS} x {WINDOWS} windows of about {WINDOW_S} s; "
            f"A = the previous library, B = this tree's, {PROCS} processes each; windows A1, B1, A2, B2, ...; the medians of the "
            "processes one by one in parentheses")
        ok = True
        for call in CALLS:
            one = max(ask(kid, 0, call) for kid in kids)
            iters = max(3, int(WINDOW_S * 1e6 / one))
            per = [[] for _ in kids]
            for _ in range(WINDOWS):
                for k, kid in enumerate(kids):
                    per[k].append(ask(kid, iters, call))
            t = [sum(per[k::2], []) for k in range(2)]      # kids alternate A, B
            ma, mb = statistics.median(t[0]), statistics.median(t[1])
            bar = ma + (max(t[0]) - min(t[0]))
            ok &= mb <= bar
            say(f"{call}, windows of {iters} calls:")
            for tag, w in zip("AB", t):
                say(f"  {tag} {statistics.median(w):9.1f} [{min(w):9.1f} .. {max(w):9.1f}]   ("
                    + ", ".join("%.1f" % statistics.median(q) for q in per["AB".index(tag)::2]) + ")   " + " ".join("%.1f" % x for x in w))
            say(f"  B / A {mb / ma:.4f}; bar = A's median + A's (max - min) = {bar:.1f}: {'within' if mb <= bar else 'ABOVE'}")
        say("ALL WITHIN THE PREVIOUS LIBRARY'S SPREAD" if ok else "A CALL IS ABOVE THE PREVIOUS LIBRARY'S SPREAD")
        for kid in kids:
            kid.stdin.close()
        for kid in kids:
            kid.wait(timeout=60)
    finally:
        for kid in kids:
            if kid.poll() is None:
                kid.kill()
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    child() if sys.argv[1] == "--child" else main()
