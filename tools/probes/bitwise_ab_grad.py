"""A/B of two builds of libcmcd_hip.so, gradient entry points (the forward's: bitwise_ab.py): one value-and-gradient call per
configuration with each library in its own process; gradient, losses and z compared with torch.equal on the bit patterns.
The previous library runs twice: a quantity it does not return with the same bits in both runs (gradient entries summed through
float atomics) is reported and those entries are left out of the comparison; only gradient entries may be — losses and z that do not reproduce are a failure.
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
# the ten whole-chain instances of grad_kernel's local gradient (BPTT = false, ITEM = false): gmm / many_gmm on geffner T = 2, 4, 9
# (widths 22, 50, 132) and dds 64, funnel on geffner T = 4 (58) and dds; n = 33 (two full tiles and a one-lane tile), K = 8, pinned to
# whole chains (CMCD_GRAD_ITEM = 0: at this size the measured rule takes work items)
VAR = {"boundmode": "MCD_CAIS_var_sn", "nbridges": 8}
CASES += [(name, dict(VAR, **over), 33, "var", "0")
          for name in ("gmm_n300_k8", "many_gmm_var_n16000_k256")
          for over in ({"emb_dim": 20}, {"emb_dim": 48}, {"emb_dim": 130}, {"nn_arch": "dds"})]
CASES += [("funnel_n300_k64", dict(VAR, **over), 33, "var", "0") for over in ({"emb_dim": 48}, {"nn_arch": "dds"})]
NAMES = ("gradient", "losses", "z")

def child(out):
    sys.path.insert(0, ROOT)
    import numpy as np, torch
    from cmcd_amd import synthetic, mcdboundingmachine as mcdbm
    res = {}
    for k, (name, over, n, kind, *item) in enumerate(CASES):
        os.environ.pop("CMCD_GRAD_ITEM", None)
        if item:
            os.environ["CMCD_GRAD_ITEM"] = item[0]
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
        for i, lib in enumerate((sys.argv[1], sys.argv[1], sys.argv[2])):
            out = os.path.join(tmp, "grad_ab_%d.pt" % i)
            subprocess.run([sys.executable, os.path.abspath(__file__), "--child", out], check=True,
                           env=dict(os.environ, CMCD_LIB_PATH=os.path.abspath(lib)), timeout=600)
            outs.append(torch.load(out))
    bits = lambda t: t.view(torch.int32) if t.dtype == torch.float32 else t
    ok = True
    for k, c in enumerate(CASES):
        verdict = []
        for q, a0, a1, b in zip(NAMES, outs[0][k], outs[1][k], outs[2][k]):
            same = bits(a0) == bits(a1)
            if not bool(same.all()):
                ok &= q == "gradient"
                verdict.append("%s: %d of %d entries NOT REPRODUCED by the previous library, left out"
                               % (q, int((~same).sum()), a0.numel()))
            if not torch.equal(bits(a0)[same], bits(b)[same]):
                ok = False
                verdict.append("%s DIFFERENT" % q)
        print(c[0], c[1], "n", c[2], c[3], "whole chains" if len(c) > 4 else "", "; ".join(verdict) or "identical", flush=True)
    print("ALL IDENTICAL" if ok else "DIFFERENCES FOUND")
    sys.exit(0 if ok else 1)
