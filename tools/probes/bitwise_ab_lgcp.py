"""A/B of two builds of libcmcd_hip.so on the d = 1600 path (cmcd_lgcp.hip, cmcd_lgcp_wide.hip; the small-d entry points:
bitwise_ab.py, bitwise_ab_grad.py): each library in its own process, the previous one twice.  Per library
  - every case of tests/lgcp_grad_cases.CASES on the dense parameter set with the case's form: the forward-only call and the
    value-and-gradient call (lc.build, lc.forward, lc.call),
  - forward-only calls at n = 33 with forms 1 (32-row passes pinned) and 2 (the wide path pinned),
  - a forward at n = 225, K = 2 (the wide path by the library's own choice);
losses, z and the flat gradient compared with torch.equal on the bit patterns.  Losses and z must reproduce in the previous
library's two runs; gradient entries that do not (float atomics: lgcp_tn_gemm_kernel's two order-free addends per address, so
none are expected) are counted, named by block and left out.
  python tools/probes/bitwise_ab_lgcp.py <previous libcmcd_hip.so> cmcd_amd/libcmcd_hip.so"""
import os, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CAIS = "MCD_CAIS_sn"
TN_BLOCKS = ("W1.state.", "W1.z.", "W1.rho.", "W2.", "W3.")      # lc.blocks names of the lgcp_tn_gemm_kernel outputs
FORWARDS = [("fwd-n33-form1", CAIS, 33, 2, 1, {}), ("fwd-n33-form2", CAIS, 33, 2, 2, {}), ("fwd-n225-wide", CAIS, 225, 2, 0, {})]


def child(out):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import torch
    import lgcp_grad_cases as lc
    from cmcd_amd import mcdboundingmachine as mcdbm
    res = {}
    for case in lc.CASES + FORWARDS:
        mcdbm.KERNEL_VARIANT = case[4]
        b = lc.build(case, "dense")
        seeds = torch.from_numpy(lc.seeds_of(case)).cuda()
        l, z = lc.forward(b, seeds)[:2]
        torch.cuda.synchronize()
        got = {"forward losses": l, "forward z": z}
        if case not in FORWARDS:
            g, (l2, z2) = lc.call(b, seeds)
            torch.cuda.synchronize()
            got.update({"gradient": g, "losses": l2, "z": z2})
        res[case[0]] = {k: t.detach().cpu() for k, t in got.items()}
        print(case[0], flush=True)
    torch.save(res, out)


def grad_blocks_of(case, mask):
    """Names of the blocks (lc.blocks) that hold the flat-gradient entries under `mask`."""
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import lgcp_grad_cases as lc
    b = lc.build(case, "dense", device="cpu")
    return sorted({name for name, a, covers in lc.blocks(b["unflatten"], mask.numpy()) if covers and a.any()})


if __name__ == "__main__":
    if sys.argv[1] == "--child":
        child(sys.argv[2]); sys.exit(0)
    import torch
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import lgcp_grad_cases as lc
    outs = []
    with tempfile.TemporaryDirectory() as tmp:
        for i, lib in enumerate((sys.argv[1], sys.argv[1], sys.argv[2])):
            out = os.path.join(tmp, "lgcp_ab_%d.pt" % i)
            subprocess.run([sys.executable, os.path.abspath(__file__), "--child", out], check=True, stdout=subprocess.DEVNULL,
                           env=dict(os.environ, CMCD_LIB_PATH=os.path.abspath(lib)), timeout=900)
            outs.append(torch.load(out))
    bits = lambda t: t.view(torch.int32) if t.dtype == torch.float32 else t
    ok = True
    for case in lc.CASES + FORWARDS:
        verdict = []
        for q in outs[0][case[0]]:
            a0, a1, b = (o[case[0]][q] for o in outs)
            same = bits(a0) == bits(a1)
            if not bool(same.all()):
                where = grad_blocks_of(case, ~same) if q == "gradient" else []
                # only what lgcp_tn_gemm_kernel's float atomics write may fail to reproduce: the state rows of W1, W2, W3
                ok &= q == "gradient" and bool(where) and all(w.startswith(TN_BLOCKS) for w in where)
                verdict.append("%s: %d of %d entries NOT REPRODUCED by the previous library, left out %s"
                               % (q, int((~same).sum()), a0.numel(), where))
            if not torch.equal(bits(a0)[same], bits(b)[same]):
                ok = False
                verdict.append("%s DIFFERENT" % q)
        print("%-14s n %3d K %d form %d  %s" % (case[0], case[2], case[3], case[4], "; ".join(verdict) or "identical"), flush=True)
    print("ALL IDENTICAL" if ok else "DIFFERENCES FOUND")
    sys.exit(0 if ok else 1)
