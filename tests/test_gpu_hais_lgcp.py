"""UHA on lgcp on the GPU — cmcd_amd.hais_lgcp over cmcd_hais_lgcp_bound_grad (cmcd_amd/csrc/cmcd_hais_lgcp.hip) — against the
float64 restatement (tests/hais_restatement.py on oracle.cmcd_oracle_torch.make_logp_lgcp), which tests/test_oracle_hais_lgcp.py
pins on the CPU.  Cases, blocks and bars: tests/hais_lgcp_cases.py.  Forward parity under helpers.compare_losses with every
element of z (K <= 32), gradient parity per block, the same bits from the forward-only and the gradient call, statistics,
shards, repeats and isolation, trainable leaves, capture, training and the command-line driver."""
import functools
import math
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import hais_lgcp_cases as hc
import hais_restatement as hr
from cmcd_amd import hais_lgcp, opt
from helpers import check_stats, compare_losses, lgcp_counts_fixture

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def built(cid, trainable=("eta", "eps", "vd", "mgridref_y", "md")):
    return hc.params(hc.case_by_id(cid), device="cuda", trainable=trainable)


def dev(seeds):
    return torch.from_numpy(np.asarray(seeds, np.int32)).cuda()


def grad_call(cid, seeds=None, **kw):
    flat, un, fixed = built(cid)
    seeds = hc.seeds_of(hc.case_by_id(cid)) if seeds is None else seeds
    g, (l, z) = hais_lgcp.grad_and_loss(dev(seeds), flat, un, fixed, hc.target(), **kw)
    torch.cuda.synchronize()
    return g, l, z


def forward_call(cid, seeds=None):
    flat, un, fixed = built(cid)
    seeds = hc.seeds_of(hc.case_by_id(cid)) if seeds is None else seeds
    out = hais_lgcp.bound_forward(dev(seeds), flat, un, fixed, hc.target())
    torch.cuda.synchronize()
    return out


def leaves(cid, g):
    return hc.leaves_of_flat(built(cid)[1], g.detach().cpu().numpy())


# ------------------------------------------------------------------------------------------ parity and the same bits
@pytest.mark.parametrize("cid", hc.IDS)
def test_forward_and_gradient_match_the_restatement(hip_lib, cid):
    case = hc.case_by_id(cid)
    l_ref, z_ref, g_ref = hc.reference(case)
    assert np.isfinite(l_ref).all()
    losses, z, stats = forward_call(cid)
    rep = compare_losses(losses.cpu().numpy(), l_ref, z.cpu().numpy(), z_ref, tag=cid, K=case[2])
    print(cid, {k: rep[k] for k in ("mean_err", "rel_max", "z_max")})
    flat, un, fixed = built(cid)
    mean, (l2, z2) = hais_lgcp.compute_bound(dev(hc.seeds_of(case)), flat, un, fixed, hc.target())
    assert torch.equal(l2, losses) and torch.equal(z2, z)
    assert abs(float(mean) - float(losses.double().mean())) <= 1e-5 * max(1.0, abs(float(mean)))
    g, l_g, z_g = grad_call(cid)
    assert torch.equal(l_g, losses) and torch.equal(z_g, z), "the gradient call returns the forward-only call's bits"
    if not case[8]:
        return
    assert torch.isfinite(g).all()
    errs, bad, lost = hc.compare_blocks(case, leaves(cid, g), g_ref, tag=cid)
    worst = max(errs, key=errs.get)
    print(cid, "blocks %d, worst %s: %.3e of its maximum" % (len(errs), worst, errs[worst]))
    assert not lost, lost                      # the stored gaps lose no block
    assert not bad, "\n".join(bad)
    # the two grids carry no gradient
    for name in ("gridref_x", "target_x"):
        off, shape = un.offset(name), un.shape(name)
        assert not g[off:off + shape[0]].any()


# ------------------------------------------------------------------------------------------ statistics
@pytest.mark.parametrize("cid", ["n1", "n33", "n65"])
def test_statistics_of_the_forward_and_the_gradient_call(hip_lib, cid):
    losses, _, stats = forward_call(cid)
    print(check_stats(stats, losses, tag=cid))
    flat, un, fixed = built(cid)
    _, l_g, _, st_g = hais_lgcp._call(dev(hc.seeds_of(hc.case_by_id(cid))), flat, un, fixed, hc.target(), True)
    print(check_stats(st_g, l_g, tag=cid + " gradient call"))
    assert torch.equal(st_g, stats)


def test_statistics_beyond_64_records(hip_lib):
    """n = 1040, K = 1, L = 1: 65 records of 16, the finalize launch beyond 64 records; against the returned losses alone."""
    flat, un, fixed = built("k1l1")
    losses, z, stats = hais_lgcp.bound_forward(dev(np.arange(1, 1041)), flat, un, fixed, hc.target())
    torch.cuda.synchronize()
    assert torch.isfinite(losses).all() and torch.isfinite(z).all()
    print(check_stats(stats, losses, tag="n1040"))
    l20, z20, _ = forward_call("k1l1")
    assert torch.equal(losses[:20], l20) and torch.equal(z[:20], z20)      # a particle's bits do not depend on the batch


# ------------------------------------------------------------------------------------------ shards
def test_shards_add_up_and_n_total_scales_bit_for_bit(hip_lib):
    seeds = hc.seeds_of(hc.case_by_id("n65"))
    g, l, z = grad_call("n65")
    ga, la, za = grad_call("n65", seeds[:33], n_total=65)
    gb, lb, zb = grad_call("n65", seeds[33:], n_total=65)
    assert torch.equal(torch.cat([la, lb]), l) and torch.equal(torch.cat([za, zb]), z)
    whole, parts = leaves("n65", g), leaves("n65", ga + gb)
    for name, (e, s) in hc.block_errors(parts, whole).items():
        assert e <= hc.SHARD_TOL * s, (name, e, s)
    g2, _, _ = grad_call("n65", n_total=130)
    assert torch.equal(g2 * 2.0, g)


# ------------------------------------------------------------------------------------------ repeats and isolation
def test_repeated_calls_and_a_smaller_call_in_between_keep_the_bits(hip_lib):
    first = grad_call("n65")
    for _ in range(5):
        again = grad_call("n65")
        assert all(torch.equal(a, b) for a, b in zip(first, again))
    small = grad_call("n65", hc.seeds_of(hc.case_by_id("n65"))[:5])      # the same stream's workspace, smaller layout
    assert torch.equal(small[1], first[1][:5])
    after = grad_call("n65")
    assert all(torch.equal(a, b) for a, b in zip(first, after))
    assert float(first[0].abs().max()) > 0


def test_reversed_seeds_give_reversed_losses_and_the_same_gradient(hip_lib):
    seeds = hc.seeds_of(hc.case_by_id("n33"))
    g, l, z = grad_call("n33")
    gr, lr, zr = grad_call("n33", seeds[::-1].copy())
    assert torch.equal(lr.flip(0), l) and torch.equal(zr.flip(0), z)
    for name, (e, s) in hc.block_errors(leaves("n33", gr), leaves("n33", g)).items():
        assert e <= hc.SHARD_TOL * s, (name, e, s)


# ------------------------------------------------------------------------------------------ trainable leaves
@pytest.mark.parametrize("trainable", [("eta",), ()])
def test_only_the_trainable_leaves_carry_a_gradient(hip_lib, trainable):
    case = hc.case_by_id("k1l1")
    flat, un, fixed = built("k1l1", trainable=trainable)
    g, (l, z) = hais_lgcp.grad_and_loss(dev(hc.seeds_of(case)), flat, un, fixed, hc.target())
    torch.cuda.synchronize()
    full, _, _ = grad_call("k1l1")
    un_full = built("k1l1")[1]
    if trainable:
        off = un.offset("eta")
        assert float(g[off]) == float(full[un_full.offset("eta")]) != 0.0
        rest = g.clone()
        rest[off] = 0.0
        assert not rest.any()
    else:
        assert not g.any()
    assert torch.equal(l, forward_call("k1l1")[0])


# ------------------------------------------------------------------------------------------ capture
@pytest.mark.parametrize("with_grad", [False, True])
def test_captured_call_replays_the_eager_bits(hip_lib, with_grad):
    case = hc.case_by_id("k1l1")
    flat, un, fixed = built("k1l1")
    tgt = hc.target()
    static = dev(hc.seeds_of(case))

    def call():
        if with_grad:
            g, (l, z) = hais_lgcp.grad_and_loss(static, flat, un, fixed, tgt)
            return g, l, z
        return hais_lgcp.bound_forward(static, flat, un, fixed, tgt)

    eager = [t.clone() for t in call()]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()                                                      # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        captured = call()
    for _ in range(3):
        for t in captured:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(captured, eager))


# ------------------------------------------------------------------------------------------ training and the driver
def test_training_lowers_the_bound(hip_lib):
    """opt.run from the reference's start (q = N(mu0, I), uniform grid, eta = 0, the default init_eps): K = 4, L = 1, N = 20,
    60 iterations at LR_DICT["lgcp"]["UHA"]."""
    from cmcd_amd.main import LR_DICT
    trainable = ("eta", "eps", "vd", "mgridref_y")
    vd = {"mean": torch.full((hc.D,), hc.MU0), "logdiag": torch.zeros(hc.D)}
    flat, un, fixed = hais_lgcp.initialize(hc.D, vdparams=vd, nbridges=4, lfsteps=1, eps=1e-5, eta=0.0, trainable=trainable,
                                           device="cuda")
    losses, trained, _ = opt.run(types.SimpleNamespace(N=20), LR_DICT["lgcp"]["UHA"], 60, flat, un, fixed, hc.target(),
                                 hais_lgcp.grad_and_loss, trainable, 7)
    torch.cuda.synchronize()
    assert len(losses) == 60 and np.isfinite(losses).all()
    first, last = float(np.mean(losses[:10])), float(np.mean(losses[-10:]))
    print("mean loss of the first 10 iterations %.3f, of the last 10 %.3f" % (first, last))
    assert last < first
    assert torch.isfinite(trained).all() and not torch.equal(trained, flat)
    eps = float(trained[un.offset("eps")])
    assert 0.0000001 <= eps <= 0.5


def test_driver_runs_uha_on_lgcp(hip_lib, tmp_path):
    """python -m cmcd_amd.main --config.model lgcp with the reference's default boundmode, on a point set written from the
    fixture's bin counts (every point at the centre of its bin), in a fresh child process."""
    counts = lgcp_counts_fixture().reshape(40, 40)
    rows = [((r + 0.5) / 40, (c + 0.5) / 40) for r in range(40) for c in range(40) for _ in range(int(counts[r, c]))]
    path = tmp_path / "points.csv"
    np.savetxt(path, np.asarray(rows), delimiter=",")
    argv = [sys.executable, "-m", "cmcd_amd.main", "--config.model", "lgcp", "--config.boundmode", "UHA", "--config.file_path", str(path),
            "--config.N", "5", "--config.nbridges", "4", "--config.mfvi_iters", "20", "--config.iters", "5",
            "--config.n_samples", "8", "--config.n_input_dist_seeds", "2", "--noconfig.compute_w2"]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run(argv, cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "Params being trained : ('eta', 'eps', 'vd', 'mgridref_y')" in out.stdout
    import re
    for pat in (r"Done training, got ELBO (\S+)\.\n", r"Done training, got ln Z (\S+)\.\n"):
        m = re.search(pat, out.stdout)
        assert m and math.isfinite(float(m.group(1))), (pat, out.stdout[-2000:])
