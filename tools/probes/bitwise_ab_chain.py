"""A/B of two builds of libcmcd_hip.so, the reverse-time chain and the chain segments (the forward's: bitwise_ab.py, the gradients':
bitwise_ab_grad.py): every instance of reverse_traj_kernel and segment_traj_kernel, then the three momentum families (2nd-order
CMCD and UHA on gmm and funnel, UHA with lfsteps = 2; LDVI on gmm with and without the network, funnel and many_gmm), once with each
library in its own process — n = 33 (two full tiles and a one-lane tile), K = 8, dense parameters; out_w / out_z0 [/ out_rho0] /
stats of the reverse call, and z [/ rho] / wpath / lg / key / stats of the segments (0, K) and (3, 6), the latter from the state
that (0, 3) left, compared with torch.equal on the bit patterns.  Each library is driven by the Python package it lies in
(<root>/cmcd_amd/libcmcd_hip.so: <root>'s cmcd_amd), so that two checkouts compare their Python halves as well; a library
outside a checkout is driven by this one's package.
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
# the momentum families: (family, configuration, overrides).  2nd-order CMCD and LDVI share the tree of MCD_CAIS_UHA_sn (the step
# sizes of tools/probes/segment_ldvi_hais_time.py); UHA takes (eps, sigma of q) and runs at lfsteps = 2
UHA_SN = {"boundmode": "MCD_CAIS_UHA_sn"}
MOMENTUM = [("uha", "gmm_n300_k8", UHA_SN), ("uha", "funnel_n300_k64", UHA_SN),
            ("ldvi", "gmm_n300_k8", UHA_SN), ("ldvi-no-net", "gmm_n300_k8", UHA_SN),
            ("ldvi", "funnel_n300_k64", dict(UHA_SN, init_eps=0.01, init_gamma=4.0)),
            ("ldvi", "many_gmm_n2000_k256_dds", dict(UHA_SN, nn_arch="geffner", emb_dim=20, init_eps=0.05, init_gamma=2.0)),
            ("hais", "gmm_n300_k8", (0.05, 2.0)), ("hais", "funnel_n300_k64", (0.02, 1.0))]
SEG = ("z", "wpath", "lg", "key", "stats")
SEG_RHO = ("z", "rho", "wpath", "lg", "key", "stats")

def child(out, root):
    sys.path.insert(0, root)
    import torch
    from cmcd_amd import synthetic, smc, mcdboundingmachine as mcdbm
    from cmcd_amd import hais, reverse_hais, reverse_ldvi, reverse_uha, smc_hais, smc_ldvi, smc_uha
    from cmcd_amd import variationaldist as vd
    from cmcd_amd.model_handler import exact_target_draws, load_model
    seeds = torch.from_numpy(synthetic.parity_seeds(N)).cuda()

    def run(reverse, segment, fields, model, dim, args, kw):
        x = torch.from_numpy(exact_target_draws(model, load_model(model, None)[2], 5, N, dim)).cuda()
        got = list(reverse(seeds, x, *args, **kw))
        whole = segment(seeds, 0, K, *args, **kw)
        mid = segment(segment(seeds, 0, 3, *args, **kw), 3, 6, *args, **kw)
        got += [s[f] for s in (whole, mid) for f in fields]
        torch.cuda.synchronize()
        return [t.detach().cpu() for t in got]

    res = {}
    for k, (name, over) in enumerate(CASES):
        b = synthetic.build(name, device="cuda", dense=True, nbridges=K, **over)
        res[k] = run(mcdbm.bound_reverse, smc.segment, SEG, b["cfg"]["model"], b["params_fixed"][0],
                     (b["params_flat"], b["unflatten"], b["params_fixed"], b["target"]),
                     dict(eps_schedule=b["eps_schedule"], grad_clipping=b["grad_clipping"]))
    for k, (family, name, over) in enumerate(MOMENTUM, len(CASES)):
        b = synthetic.build(name, device="cuda", dense=True, nbridges=K, **(over if family != "hais" else {}))
        dim, _, _, spec = b["params_fixed"]
        if family == "hais":
            flat, un, fixed = hais.initialize(dim=dim, nbridges=K, lfsteps=2, eps=over[0], eta=0.5, device="cuda",
                                              vdparams=vd.initialize(dim, init_sigma=over[1]), trainable=("eta", "eps", "vd", "mgridref_y"))
            res[k] = run(reverse_hais.bound_reverse, smc_hais.segment, SEG_RHO, b["cfg"]["model"], dim, (flat, un, fixed, b["target"]), {})
        elif family == "uha":
            res[k] = run(reverse_uha.bound_reverse, smc_uha.segment, SEG_RHO, b["cfg"]["model"], dim,
                         (b["params_flat"], b["unflatten"], b["params_fixed"], b["target"]), {})
        else:
            fixed = (dim, K, "MCD_U_a-lp-sn" if family == "ldvi" else "MCD_U_a-lp", spec)
            res[k] = run(reverse_ldvi.bound_reverse, smc_ldvi.segment, SEG_RHO, b["cfg"]["model"], dim,
                         (b["params_flat"], b["unflatten"], fixed, b["target"]), {})
    torch.save(res, out)

def bits(t):
    import torch
    return t.view(torch.int32) if t.dtype == torch.float32 else (t.view(torch.int64) if t.dtype == torch.float64 else t)

if __name__ == "__main__":
    if sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3]); sys.exit(0)
    import torch
    outs = []
    with tempfile.TemporaryDirectory() as tmp:
        for i, lib in enumerate(sys.argv[1:3]):
            out = os.path.join(tmp, "chain_ab_%d.pt" % i)
            root = os.path.dirname(os.path.dirname(os.path.abspath(lib)))
            root = root if os.path.exists(os.path.join(root, "cmcd_amd", "__init__.py")) else ROOT
            print("library", os.path.abspath(lib), "driven by the package in", root, flush=True)
            subprocess.run([sys.executable, os.path.abspath(__file__), "--child", out, root], check=True,
                           env=dict(os.environ, CMCD_LIB_PATH=os.path.abspath(lib)), timeout=300)
            outs.append(torch.load(out))
    ok = True
    for k, c in enumerate(CASES + MOMENTUM):
        want = 3 + 2 * len(SEG) if k < len(CASES) else 4 + 2 * len(SEG_RHO)
        same = len(outs[0][k]) == len(outs[1][k]) == want and \
            all(torch.equal(bits(x), bits(y)) for x, y in zip(outs[0][k], outs[1][k]))
        ok &= same
        print(*c, "n", N, "K", K, "reverse + segments (0, K), (3, 6):", "identical" if same else "DIFFERENT", flush=True)
    print("ALL IDENTICAL" if ok else "DIFFERENCES FOUND")
    sys.exit(0 if ok else 1)
