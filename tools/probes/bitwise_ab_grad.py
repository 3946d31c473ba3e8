"""A/B of two builds of libcmcd_hip.so, gradient entry points (the forward's: bitwise_ab.py): one value-and-gradient call per
configuration with each library in its own process; gradient, losses and z compared with torch.equal on the bit patterns.
  python tools/probes/bitwise_ab_grad.py <previous libcmcd_hip.so> cmcd_amd/libcmcd_hip.so"""
import os, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CASES = [("gmm_n300_k8", {}, 300, "sn"), ("many_gmm_n2000_k256_dds", {"nbridges": 32}, 2000, "sn"),
         ("funnel_n300_k64", {}, 300, "sn"), ("gmm_n300_k8", {"boundmode": "MCD_ULA"}, 300, "sn"),
         ("gmm_n300_k8", {"boundmode": "MCD_ULA_sn"}, 300, "sn"),
         ("funnel_n300_k64", {"boundmode": "MCD_CAIS_UHA_sn", "init_gamma": 2.0}, 300, "sn"),
         ("many_gmm_var_n16000_k256", {"nbridges": 32}, 2000, "var"), ("many_gmm_var_n16000_k256", {"nbridges": 32}, 300, "var"),
         ("gmm_n300_k8", {"boundmode": "MCD_CAIS_var_sn"}, 300, "var"),
         ("lgcp_n20_k128", {"nbridges": 8}, 20, "sn"), ("lgcp_n20_k128", {"nbridges": 8, "boundmode": "MCD_CAIS_var_sn"}, 20, "var")]

def child(out):
    sys.path.insert(0, ROOT)
    import numpy as np, torch
    from cmcd_amd import synthetic, mcdboundingmachine as mcdbm
    res = {}
    for k, (name, over, n, kind) in enumerate(CASES):
        if "lgcp" in name:
            over = dict(over, lgcp_counts=np.load(os.path.join(ROOT, "tests", "golden", "lgcp_bin_counts.npy")))
        b = synthetic.build(name, device="cuda", dense=True, **over)
        seeds = torch.from_numpy(synthetic.parity_seeds(n)).cuda()
        fn = mcdbm.compute_bound_grad if kind == "sn" else mcdbm.compute_log_var_grad
        g, (l, z) = fn(seeds, b["params_flat"], b["unflatten"], b["params_fixed"], b["target"],
                       eps_schedule=b["eps_schedule"], grad_clipping=b["grad_clipping"])
        torch.cuda.synchronize()
        res[k] = [t.detach().cpu() for t in (g, l, z)]
    torch.save(res, out)

if __name__ == "__main__":
    if sys.argv[1] == "--child":
        child(sys.argv[2]); sys.exit(0)
    import torch
    outs = []
    with tempfile.TemporaryDirectory() as tmp:
        for i, lib in enumerate(sys.argv[1:3]):
            out = os.path.join(tmp, "grad_ab_%d.pt" % i)
            subprocess.run([sys.executable, os.path.abspath(__file__), "--child", out], check=True,
                           env=dict(os.environ, CMCD_LIB_PATH=os.path.abspath(lib)), timeout=600)
            outs.append(torch.load(out))
    ok = True
    for k, c in enumerate(CASES):
        same = all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)
                   for x, y in zip(outs[0][k], outs[1][k]))
        ok &= same
        print(c[0], {a: b for a, b in c[1].items()}, c[2], c[3], "identical" if same else "DIFFERENT", flush=True)
    print("ALL IDENTICAL" if ok else "DIFFERENCES FOUND")
    sys.exit(0 if ok else 1)
