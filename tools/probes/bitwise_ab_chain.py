"""A/B of two builds of libcmcd_hip.so, the reverse-time chain and the chain segments (the forward's: bitwise_ab.py, the gradients':
bitwise_ab_grad.py): every instance of reverse_traj_kernel and segment_traj_kernel once with each library in its own process —
n = 33 (two full tiles and a one-lane tile), K = 8, dense parameters; out_w / out_z0 / stats of the reverse call, and z / wpath /
lg / key / stats of the segments (0, K) and (3, 6), the latter from the state that (0, 3) left, compared with torch.equal on the
bit patterns.
  python tools/probes/bitwise_ab_chain.py <previous libcmcd_hip.so> cmcd_amd/libcmcd_hip.so"""
import os, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
N, K = 33, 8
# the eleven instances: gmm / many_gmm on geffner T = 2, 4, 9 (widths 22, 50, 132) and dds 64, funnel on geffner T = 4, 9 (58, 132)
# and dds; the many_gmm geffner cases are the VarGrad mode with clipping on (both clips act); then MCD_ULA and MCD_ULA_sn on gmm
CASES = [("gmm_n300_k8", {}), ("gmm_n300_k8", {"emb_dim": 48}), ("gmm_n300_k8", {"emb_dim": 130}), ("gmm_n300_k8", {"nn_arch": "dds"}),
         ("many_gmm_var_n16000_k256", {"emb_dim": 20}), ("many_gmm_var_n16000_k256", {"emb_dim": 48}),
         ("many_gmm_var_n16000_k256", {}), ("many_gmm_n2000_k256_dds", {}),
         ("funnel_n300_k64", {}), ("funnel_n300_k64", {"emb_dim": 122}), ("funnel_n300_k64", {"nn_arch": "dds"}),
         ("gmm_n300_k8", {"boundmode": "MCD_ULA"}), ("gmm_n300_k8", {"boundmode": "MCD_ULA_sn"})]
SEG = ("z", "wpath", "lg", "key", "stats")

def child(out):
    sys.path.insert(0, ROOT)
    import torch
    from cmcd_amd import synthetic, smc, mcdboundingmachine as mcdbm
    from cmcd_amd.model_handler import exact_target_draws, load_model
    res = {}
    for k, (name, over) in enumerate(CASES):
        b = synthetic.build(name, device="cuda", dense=True, nbridges=K, **over)
        cfg = b["cfg"]
        seeds = torch.from_numpy(synthetic.parity_seeds(N)).cuda()
        x = torch.from_numpy(exact_target_draws(cfg["model"], load_model(cfg["model"], None)[2], 5, N, b["params_fixed"][0])).cuda()
        args = (b["params_flat"], b["unflatten"], b["params_fixed"], b["target"])
        kw = dict(eps_schedule=b["eps_schedule"], grad_clipping=b["grad_clipping"])
        got = list(mcdbm.bound_reverse(seeds, x, *args, **kw))
        whole = smc.segment(seeds, 0, K, *args, **kw)
        mid = smc.segment(smc.segment(seeds, 0, 3, *args, **kw), 3, 6, *args, **kw)
        got += [s[f] for s in (whole, mid) for f in SEG]
        torch.cuda.synchronize()
        res[k] = [t.detach().cpu() for t in got]
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
        for i, lib in enumerate(sys.argv[1:3]):
            out = os.path.join(tmp, "chain_ab_%d.pt" % i)
            subprocess.run([sys.executable, os.path.abspath(__file__), "--child", out], check=True,
                           env=dict(os.environ, CMCD_LIB_PATH=os.path.abspath(lib)), timeout=300)
            outs.append(torch.load(out))
    ok = True
    for k, c in enumerate(CASES):
        same = len(outs[0][k]) == len(outs[1][k]) == 3 + 2 * len(SEG) and \
            all(torch.equal(bits(x), bits(y)) for x, y in zip(outs[0][k], outs[1][k]))
        ok &= same
        print(c[0], c[1], "n", N, "K", K, "reverse + segments (0, K), (3, 6):", "identical" if same else "DIFFERENT", flush=True)
    print("ALL IDENTICAL" if ok else "DIFFERENCES FOUND")
    sys.exit(0 if ok else 1)
