"""A/B of two builds of libcmcd_hip.so, the network-free wave-per-tile kernels (the gradients': bitwise_ab_grad.py, the chains':
bitwise_ab_chain.py): cmcd_mfvi_bound_grad (mfvi_kernel) and cmcd_hais_bound_grad with K = 8, L = 2 (hais_traj_kernel,
hais_grad_kernel, hais_reduce_kernel) on gmm, many_gmm and funnel, n = 33 (two full tiles and a one-lane tile), every parameter
leaf non-trivial (tests/hais_restatement.make_params); each library in its own process.  Gradient, losses, z and the five
statistics compared with torch.equal on the bit patterns.  The previous library runs twice: what it does not return with the
same bits in both runs is reported and left out — no kernel here has float atomics, so anything reported is a failure.
  python tools/probes/bitwise_ab_plain.py <previous libcmcd_hip.so> cmcd_amd/libcmcd_hip.so"""
import os, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
N, K, L = 33, 8, 2
# (target, eps, q's sigma, scale of q's mean): the parameter sets of tests/test_gpu_hais.py
TARGETS = [("gmm", 0.05, 2.0, 1.0), ("many_gmm", 0.1, 15.0, 5.0), ("funnel", 0.05, 1.0, 0.5)]
CALLS = ("mfvi", "hais")
NAMES = ("gradient", "losses", "z", "stats")

def child(out):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np, torch
    import hais_restatement as hr
    from cmcd_amd import boundingmachine as bm, hais, model_handler
    res = {}
    seeds = torch.from_numpy(np.arange(1, N + 1, dtype=np.int32)).cuda()
    for name, eps, sigma, mean_scale in TARGETS:
        tgt = model_handler.load_model(name)[0]
        flat, un, fixed = hr.make_params(tgt.dim, K, L, eps, seed=K + 10 * L, device="cuda", mean_scale=mean_scale, sigma=sigma)
        for call in CALLS:
            if call == "mfvi":
                got = bm._call(seeds, flat, un, (tgt.dim, 0, 1), tgt, True)
            else:
                got = hais._call(seeds, flat, un, fixed, tgt, True)
            torch.cuda.synchronize()
            res[name, call] = [t.detach().cpu() for t in got]
    torch.save(res, out)

def bits(t):
    import torch
    return t.view(torch.int32) if t.dtype == torch.float32 else (t.view(torch.int64) if t.dtype == torch.float64 else t)

if __name__ == "__main__":
    if sys.argv[1] == "--child":
        child(sys.argv[2]); sys.exit(0)
    import torch
    outs = []
    with tempfile.TemporaryDirectory() as tmp:
        for i, lib in enumerate((sys.argv[1], sys.argv[1], sys.argv[2])):
            out = os.path.join(tmp, "plain_ab_%d.pt" % i)
            subprocess.run([sys.executable, os.path.abspath(__file__), "--child", out], check=True,
                           env=dict(os.environ, CMCD_LIB_PATH=os.path.abspath(lib)), timeout=300)
            outs.append(torch.load(out))
    ok = True
    for name, *_ in TARGETS:
        for call in CALLS:
            verdict = []
            for q, a0, a1, b in zip(NAMES, outs[0][name, call], outs[1][name, call], outs[2][name, call]):
                same = bits(a0) == bits(a1)
                if not bool(same.all()):
                    ok = False
                    verdict.append("%s: %d of %d entries NOT REPRODUCED by the previous library" % (q, int((~same).sum()), a0.numel()))
                if not torch.equal(bits(a0)[same], bits(b)[same]):
                    ok = False
                    verdict.append("%s DIFFERENT" % q)
            print(name, call, "n", N, "K, L = %d, %d" % (K, L) if call == "hais" else "", "gradient, losses, z, stats:",
                  "; ".join(verdict) or "identical", flush=True)
    print("ALL IDENTICAL" if ok else "DIFFERENCES FOUND")
    sys.exit(0 if ok else 1)
