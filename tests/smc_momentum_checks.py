"""The bodies of the GPU checks that tests/test_gpu_smc_ldvi.py and tests/test_gpu_smc_hais.py share: the items of
tests/test_gpu_smc_uha.py, written once for a state with momentum and handed a `Kit` that says which module runs the segments
and which float64 restatement it is held to.  TEST INFRASTRUCTURE ONLY; nothing here is collected by pytest.

A `b` is whatever the kit's callables understand (a build() dict for LDVI, a make_params record for UHA); the checks never look
inside it."""
import math
from dataclasses import dataclass
from typing import Any, Callable

import numpy as np
import torch

from cmcd_amd import resample, synthetic
from helpers import check_stats, compare_losses
from smc_uha_restatement import losses_of as ref_losses_of
from smc_uha_restatement import smc_chain

FIELDS = ("z", "rho", "wpath", "lg", "key")


@dataclass
class Kit:
    smc: Any                    # cmcd_amd.smc_ldvi / cmcd_amd.smc_hais
    args_of: Callable           # b -> the arguments of smc.segment after (state, k0, k1)
    runner: Callable            # b -> run_segment(state, k0, k1) of the float64 restatement
    K_of: Callable              # b -> nbridges
    forward: Callable           # (b, device seeds) -> (losses, z) of the forward call of the mode


# --------------------------------------------------------------------------- plumbing
def dev_seeds(seeds):
    return torch.from_numpy(np.asarray(seeds, np.int32)).cuda()


def f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def to_device(state):
    """A restatement state, rounded to float32, as the device's state dict."""
    key = np.ascontiguousarray(state["key"], np.uint32).view(np.int32)
    return {"z": f32(state["z"]), "rho": f32(state["rho"]), "wpath": f32(state["wpath"]), "key": torch.from_numpy(key).cuda(),
            "k": state["k"]}


def rounded(state):
    """The same state as the restatement continues from: float32 values in float64 arrays."""
    r = lambda a: a.astype(np.float32).astype(np.float64)
    return dict(state, z=r(state["z"]), rho=r(state["rho"]), wpath=r(state["wpath"]))


def key_words(state):
    return state["key"].cpu().numpy().view(np.uint32)


def bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64) if t.is_floating_point() else t


def same_bits(a, b, fields=FIELDS):
    return all(torch.equal(bits(a[f]), bits(b[f])) for f in fields)


def run_device(kit, b, state, k0, k1):
    out = kit.smc.segment(state, k0, k1, *kit.args_of(b))
    torch.cuda.synchronize()
    return out


def forward_key(seeds, K):
    """gen_K of the forward chains with momentum (oracle/prng.py: particle_noise_uha), computed on the CPU."""
    from oracle import prng
    _, bb = prng.split(prng.prng_key(np.asarray(seeds)))
    c, _ = prng.split(bb)
    _, g1 = prng.split(c)
    _, gen = prng.split(g1)
    for _ in range(K):
        _, h = prng.split(gen)
        _, gen = prng.split(h)
    return gen


# --------------------------------------------------------------------------- 1. parity
def check_parity(kit, b, tag, seeds, k0, k1):
    """helpers.compare_losses / check_stats unchanged, with -(wpath + lg) in the place of the loss; wpath, lg and rho to the bars of
    tests/test_gpu_smc_uha.py; the -inf set of lg and the key words exactly.  A segment with k0 > 0 starts from the restatement's
    float32-rounded state."""
    run = kit.runner(b)
    if k0 == 0:
        start_ref, start_dev = seeds, dev_seeds(seeds)
    else:
        start_ref = rounded(run(seeds, 0, k0))
        start_dev = to_device(start_ref)
    ref = run(start_ref, k0, k1)
    out = run_device(kit, b, start_dev, k0, k1)
    lg, lg_ref = out["lg"].cpu().numpy(), ref["lg"]
    assert not np.isnan(lg).any() and not (lg == np.inf).any()
    assert np.array_equal(lg == -np.inf, lg_ref == -np.inf), f"{tag}: -inf sets of lg differ"
    assert np.array_equal(key_words(out), ref["key"]), f"{tag}: chain key"
    loss = kit.smc.losses_of(out).cpu().numpy()
    print(tag, "loss[:4]", loss[:4], "ref", ref_losses_of(ref)[:4])
    print(tag, compare_losses(loss, ref_losses_of(ref), out["z"].cpu().numpy(), ref["z"], tag, K=k1 - k0))
    fin = np.isfinite(lg_ref)
    werr = np.abs(out["wpath"].cpu().numpy() - ref["wpath"]) / np.maximum(1.0, np.abs(ref["wpath"]))
    lerr = np.abs(lg[fin] - lg_ref[fin]) / np.maximum(1.0, np.abs(lg_ref[fin]))
    print(tag, "wpath rel", werr.max(), "lg rel", lerr.max() if fin.any() else 0.0)
    bound = 1e-3 if k1 - k0 <= 32 else 0.2            # compare_losses' worst-particle bars, on the two addends
    assert werr.max() <= bound and (not fin.any() or lerr.max() <= bound)
    # rho to the bar compare_losses holds z to: p99 within 1e-3 of the scale, and every element for chains of <= 32 bridges
    rho, rho_ref = out["rho"].cpu().numpy().astype(np.float64), ref["rho"]
    f = np.isfinite(ref_losses_of(ref))
    rerr = np.abs(rho - rho_ref)[f]
    r_scale = max(1.0, float(np.quantile(np.abs(rho_ref[f]), 0.99)))
    print(tag, "rho p99", float(np.quantile(rerr, 0.99)), "max", float(rerr.max()), "scale", r_scale)
    assert not np.isnan(rho[f]).any() and np.quantile(rerr, 0.99) <= 1e-3 * r_scale
    if k1 - k0 <= 32:
        assert rerr.max() <= 1e-3 * r_scale
    print(tag, check_stats(out["stats"], kit.smc.losses_of(out), tag))


def float32_gap(kit_runner32, kit_runner64, seeds, k0, k1):
    """The restatement in float32 against the restatement in float64 on one parity case, through compare_losses' default bars (it
    raises when the case is outside them) -> dict(rel_max, z, rho, wpath, lg: worst gaps relative to their scales)."""
    outs = []
    for run in (kit_runner32, kit_runner64):
        start = seeds if k0 == 0 else rounded(kit_runner64(seeds, 0, k0))
        outs.append(run(start, k0, k1))
    a, r = outs
    assert np.array_equal(a["lg"] == -np.inf, r["lg"] == -np.inf) and np.array_equal(a["key"], r["key"])
    rep = compare_losses(ref_losses_of(a), ref_losses_of(r), a["z"], r["z"], "float32 restatement", K=k1 - k0)
    f = np.isfinite(ref_losses_of(r))
    scale = lambda x: max(1.0, float(np.quantile(np.abs(x[f]), 0.99)))
    rel = lambda x, y: float((np.abs(x - y)[f] / np.maximum(1.0, np.abs(y[f]))).max())
    return dict(rel_max=rep["rel_max"], z=rep["z_max"] / rep["z_scale"],
                rho=float(np.abs(a["rho"].astype(np.float64) - r["rho"])[f].max()) / scale(r["rho"]),
                wpath=rel(a["wpath"].astype(np.float64), r["wpath"]), lg=rel(a["lg"].astype(np.float64), r["lg"]))


# --------------------------------------------------------------------------- 2, 3. composition bits and the key
def check_composition(kit, b, seeds, full):
    K = kit.K_of(b)
    for k in sorted({1, K // 2, K - 1}):
        head = run_device(kit, b, dev_seeds(seeds), 0, k)
        assert np.array_equal(key_words(head), forward_key(seeds, k)), f"key leaving [0, {k})"
        tail = run_device(kit, b, head, k, K)
        assert same_bits(tail, full), f"[0, {k}) + [{k}, {K}) != [0, {K})"
        assert torch.equal(bits(tail["stats"]), bits(full["stats"]))
    assert np.array_equal(key_words(full), forward_key(seeds, K))


# --------------------------------------------------------------------------- 4. the forward call
def check_against_the_forward_call(kit, b, n, tag):
    K = kit.K_of(b)
    seeds = dev_seeds(synthetic.parity_seeds(n))
    out = run_device(kit, b, seeds, 0, K)
    loss_f, z_f = kit.forward(b, seeds)
    torch.cuda.synchronize()
    loss = kit.smc.losses_of(out)
    assert torch.equal(torch.isinf(loss), torch.isinf(loss_f)) and bool((loss[torch.isinf(loss)] > 0).all())
    print(tag, "bits equal to the forward call:", torch.equal(bits(loss), bits(loss_f)), torch.equal(bits(out["z"]), bits(z_f)))
    print(tag, compare_losses(loss.cpu().numpy(), loss_f.cpu().numpy(), out["z"].cpu().numpy(), z_f.cpu().numpy(), tag, K=K))
    print(tag, check_stats(out["stats"], loss, tag))


# --------------------------------------------------------------------------- 5. invariances
def make_staged(kit, b):
    """K = 8, 304 particles in 2 groups: the state at bridge 3 and one stage from it (resample, then bridges [3, 6))."""
    seeds = dev_seeds(synthetic.parity_seeds(304))
    head = run_device(kit, b, seeds, 0, 3)

    def stage(state):
        new, info = kit.smc.resample_stage(state, groups=2, ess_threshold=1.0, seed=11)
        return kit.smc.segment(new, 3, 6, *kit.args_of(b)), info

    out, info = stage(head)
    torch.cuda.synchronize()
    return b, seeds, head, stage, out, info


def check_repeated_calls(kit, staged):
    b, seeds, head, stage, out, info = staged
    again = run_device(kit, b, seeds, 0, 3)
    assert same_bits(again, head) and torch.equal(bits(again["stats"]), bits(head["stats"]))
    out2, info2 = stage(head)
    torch.cuda.synchronize()
    assert same_bits(out2, out) and torch.equal(info2["ancestors"], info["ancestors"])


def check_batch_independence(kit, staged):
    b, seeds, head, _, _, _ = staged
    rows = torch.arange(100, 117, device="cuda")       # 17 rows that straddle two tiles of the large batch
    part = run_device(kit, b, seeds[rows].contiguous(), 0, 3)
    assert all(torch.equal(bits(part[f]), bits(head[f][rows])) for f in FIELDS)
    sub = {f: head[f][rows].contiguous() for f in ("z", "rho", "wpath", "key")}
    cont, full = run_device(kit, b, sub, 3, 8), run_device(kit, b, head, 3, 8)
    assert all(torch.equal(bits(cont[f]), bits(full[f][rows])) for f in FIELDS)


def check_stage_moves_rho_with_z(kit, staged):
    b, seeds, head, stage, out, info = staged
    before = {f: head[f].clone() for f in FIELDS}
    new, info2 = kit.smc.resample_stage(head, groups=2, ess_threshold=1.0, seed=11)
    torch.cuda.synchronize()
    anc = info2["ancestors"]
    assert bool(info2["resampled"].all()) and not torch.equal(anc, torch.arange(304, device="cuda"))
    assert torch.equal(bits(new["z"]), bits(head["z"][anc])) and torch.equal(bits(new["rho"]), bits(head["rho"][anc]))
    assert torch.equal(new["key"], head["key"])                      # keys stay with their slot
    assert torch.equal(bits(new["wpath"]), bits(-head["lg"][anc])) and torch.equal(bits(new["lg"]), bits(head["lg"][anc]))
    assert same_bits(head, before)


def check_side_stream(kit, staged):
    b, seeds, head, stage, out, _ = staged
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got, _ = stage(head)
    side.synchronize()
    assert same_bits(got, out)


def check_capture(kit, staged):
    b, seeds, head, stage, out, info = staged
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        stage(head)      # allocator warm-up on a side stream
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured, cinfo = stage(head)
    for f in FIELDS:
        captured[f].zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(captured, out)
    assert torch.equal(cinfo["ancestors"], info["ancestors"]) and torch.equal(cinfo["resampled"], info["resampled"])
    assert bool(info["resampled"].all())


# --------------------------------------------------------------------------- 6. the driver, step by step
def check_driver(kit, b):
    """smc_bound against the same steps taken by hand on the device, and stage by stage against the restatement (gmm, K = 8, 3 groups
    of 48, cuts [2, 5, 7], threshold 0.9): the restatement's driver runs on the same seeds and chooses the same ancestors at every
    stage (they are decided by float64 sums of float32-close weights), so z and rho of the final state followed the same ancestors."""
    smc, args = kit.smc, kit.args_of(b)
    K, groups, m = 8, 3, 48
    assert kit.K_of(b) == K
    host_seeds = synthetic.parity_seeds(groups * m)
    seeds = dev_seeds(host_seeds)
    cuts, thr, seed = [2, 5, 7], 0.9, 4
    out = smc.smc_bound(seeds, *args, groups=groups, cuts=cuts, ess_threshold=thr, seed=seed, trace=True)
    state = smc.segment(seeds, 0, cuts[0], *args)
    acc = np.zeros(groups)
    events = []
    for i, c in enumerate(cuts):
        tr = out["trace"][i]
        assert tr["k"] == c and torch.equal(bits(tr["wpath"]), bits(state["wpath"])) and torch.equal(bits(tr["lg"]), bits(state["lg"]))
        loss = smc.losses_of(state)
        _, index, st = resample.resample(loss, state["z"], groups=groups, seed=seed + c)
        trig = (st["ess"] < thr * m) & (st["diverged"] == 0)
        events.append(trig)
        mask = trig.repeat_interleave(m)
        anc = torch.where(mask, index.long(), torch.arange(groups * m, device="cuda"))
        assert torch.equal(tr["ancestors"], anc)
        w64 = (tr["wpath"].double() + tr["lg"].double()).cpu().numpy().reshape(groups, m)
        col = np.array([np.log(np.exp(r - r.max()).sum()) + r.max() - np.log(m) for r in w64])
        acc += np.where(trig.cpu().numpy(), col, 0.0)
        state = dict(state, z=state["z"][anc], rho=state["rho"][anc], lg=state["lg"][anc],
                     wpath=torch.where(mask, -state["lg"][anc], state["wpath"]))
        state = smc.segment(state, c, cuts[i + 1] if i + 1 < len(cuts) else K, *args)
    torch.cuda.synchronize()
    assert torch.equal(out["resampled"], torch.stack(events)) and bool(out["resampled"].any())
    assert torch.equal(bits(out["losses"]), bits(smc.losses_of(state))) and torch.equal(bits(out["z"]), bits(state["z"]))
    assert torch.equal(bits(out["rho"]), bits(state["rho"]))
    last = out["trace"][-1]
    assert last["k"] == K and last["ancestors"] is None
    w64 = (last["wpath"].double() + last["lg"].double()).cpu().numpy().reshape(groups, m)
    want = acc + np.array([np.log(np.exp(r - r.max()).sum()) + r.max() - np.log(m) for r in w64])
    assert np.abs(out["ln_Z"].cpu().numpy() - want).max() <= 1e-9
    assert out["ess"].shape == (len(cuts) + 1, groups) and out["ln_Z"].dtype == torch.float64
    # the restatement's driver on the same seeds
    ref = smc_chain(host_seeds, kit.runner(b), K, groups=groups, cuts=cuts, ess_threshold=thr, seed=seed)
    ess = out["ess"].cpu().numpy()
    print("ess", ess, "ref", ref["ess"], "ln Z", out["ln_Z"].tolist(), "ref", ref["ln_Z"])
    # the first cut is reached without a resampling stage.  compare_losses lets a loss be off by d = 1e-3 max(1, |l|); every weight
    # then moves by a factor within exp(+-d), (sum w)^2 and sum w^2 by exp(+-2 d) each, the ESS by exp(+-4 d)
    l0 = ref_losses_of(ref["arrived"][0])
    d = 1e-3 * max(1.0, float(np.abs(l0[np.isfinite(l0)]).max()))
    assert np.all(np.abs(ess[0] - ref["ess"][0]) <= ref["ess"][0] * (np.exp(4 * d) - 1.0))
    same = np.array_equal(out["resampled"].cpu().numpy(), ref["resampled"]) and \
        all(np.array_equal(out["trace"][i]["ancestors"].cpu().numpy(), ref["ancestors"][i]) for i in range(len(cuts)))
    print("events and ancestors equal at every stage:", same)
    assert same      # (fixed seeds; a change here means the weights at a cut moved)
    compare_losses(out["losses"].cpu().numpy(), ref["losses"], out["z"].cpu().numpy(), ref["z"], "driver", K=K)
    assert np.abs(out["rho"].cpu().numpy() - ref["rho"]).max() <= 1e-3 * max(1.0, float(np.quantile(np.abs(ref["rho"]), 0.99)))
    assert np.abs(out["ln_Z"].cpu().numpy() - ref["ln_Z"]).max() <= 1e-3 * max(1.0, np.abs(ref["ln_Z"]).max())


def check_driver_without_resampling(kit, b, seeds, full):
    smc, args = kit.smc, kit.args_of(b)
    K = kit.K_of(b)
    out = smc.smc_bound(dev_seeds(seeds), *args, groups=1, cuts=sorted({1, K // 2, K - 1}), ess_threshold=0.0)
    torch.cuda.synchronize()
    assert not bool(out["resampled"].any())
    assert torch.equal(bits(out["losses"]), bits(smc.losses_of(full))) and torch.equal(bits(out["z"]), bits(full["z"]))
    assert torch.equal(bits(out["rho"]), bits(full["rho"]))
    column = resample.importance_stats(smc.losses_of(full), 1)["ln_Z"]
    assert torch.equal(bits(out["ln_Z"]), bits(column))
    default = smc.smc_bound(dev_seeds(seeds), *args, ess_threshold=0.0)      # the default cuts
    assert default["resampled"].shape[0] == len(smc.default_cuts(K)) and torch.equal(bits(default["losses"]), bits(out["losses"]))


# --------------------------------------------------------------------------- 7. floor particles
def check_floor(kit, b, seeds, cuts, resample_seed):
    n, groups = len(seeds), 2
    out = kit.smc.smc_bound(dev_seeds(seeds), *kit.args_of(b), groups=groups, cuts=cuts, ess_threshold=1.0, seed=resample_seed,
                            trace=True)
    torch.cuda.synchronize()
    first = out["trace"][0]
    n_floor = int((first["lg"] == -np.inf).sum())
    print("lg = -inf at the first cut:", n_floor, "events", out["resampled"].sum(0).tolist(), "ln Z", out["ln_Z"].tolist())
    assert n_floor >= 1
    for t in out["trace"]:
        assert not bool(torch.isnan(t["wpath"]).any()) and not bool(torch.isnan(t["lg"]).any())
    for name in ("ln_Z", "losses", "z", "rho", "ess"):
        assert not bool(torch.isnan(out[name]).any()), name
    hit = out["resampled"].any(0).repeat_interleave(n // groups)
    assert bool(hit.any()) and bool(torch.isfinite(out["losses"][hit]).all())
    anc = first["ancestors"].cpu().numpy()
    counts = np.bincount(anc, minlength=n)
    assert counts.max() >= 2
    slots = np.flatnonzero(anc == counts.argmax())[:2]
    z = out["z"].cpu().numpy()
    assert not np.array_equal(z[slots[0]], z[slots[1]])      # keys stay with their slot: the two offspring drew different noise


# --------------------------------------------------------------------------- 8. unbiasedness
def check_unbiased(kit, b, seeds, groups, resample_seed):
    """gmm is normalised (Z = 1): the mean over the independent particle systems of exp(ln Z_g) is 1 within 4 standard errors."""
    K = kit.K_of(b)
    out = kit.smc.smc_bound(dev_seeds(seeds), *kit.args_of(b), groups=groups, cuts=list(range(1, K)), ess_threshold=0.5,
                            seed=resample_seed)
    torch.cuda.synchronize()
    zhat = np.exp(out["ln_Z"].cpu().numpy())
    se = zhat.std(ddof=1) / np.sqrt(groups)
    print("mean exp(ln Z) %.4f, std %.4f, |mean - 1| = %.2f se, events %d" % (zhat.mean(), zhat.std(ddof=1), abs(zhat.mean() - 1) / se,
                                                                           int(out["resampled"].sum())))
    assert bool(out["resampled"].any())
    assert abs(zhat.mean() - 1.0) <= 4.0 * se


# --------------------------------------------------------------------------- 9. the NaN rule
def check_nan_rule(kit, b):
    smc, args = kit.smc, kit.args_of(b)
    groups, m, K = 3, 32, 8
    assert kit.K_of(b) == K
    seeds = dev_seeds(synthetic.parity_seeds(groups * m))
    head = run_device(kit, b, seeds, 0, 4)
    bad = dict(head, wpath=head["wpath"].clone())
    bad["wpath"][m + 5] = float("nan")                 # group 1

    def rest(state):
        new, info = smc.resample_stage(state, groups=groups, ess_threshold=1.0, seed=2)
        end = smc.segment(new, 4, K, *args)
        return info, end, resample.importance_stats(smc.losses_of(end), groups)["ln_Z"] + info["ln_Z_increment"]

    info_c, end_c, lnz_c = rest(head)
    info_b, end_b, lnz_b = rest(bad)
    torch.cuda.synchronize()
    assert info_b["resampled"].tolist() == [True, False, True] and info_c["resampled"].tolist() == [True, True, True]
    assert torch.equal(info_b["ancestors"][m:2 * m], torch.arange(m, 2 * m, device="cuda"))
    assert bool(torch.isnan(lnz_b[1])) and bool(torch.isnan(end_b["wpath"][m + 5]))
    others = torch.cat([torch.arange(0, m), torch.arange(2 * m, 3 * m)]).cuda()
    assert all(torch.equal(bits(end_b[f][others]), bits(end_c[f][others])) for f in FIELDS)
    assert torch.equal(bits(lnz_b[[0, 2]]), bits(lnz_c[[0, 2]]))


# --------------------------------------------------------------------------- the evaluation driver
def check_command_line(boundmode, capsys, smc, extra=()):
    """cli.main with --config.smc_eval prints exactly one `SMC: ln Z` line with finite figures (gmm, N = 16, K = 4, 20 iterations)."""
    from cmcd_amd import main as cli
    from cmcd_amd import utils
    argv = ["--config.model", "gmm", "--config.boundmode", boundmode, "--config.N", "16", "--config.nbridges", "4",
            "--config.mfvi_iters", "20", "--config.iters", "20", "--config.n_samples", "32", "--config.n_input_dist_seeds", "3",
            "--config.init_eps", "0.01", "--config.lr", "0.001", "--noconfig.compute_w2", "--config.smc_eval", *extra]
    utils.log_smc_diagnostics.last = {}
    elbo, ln_z = cli.main(cli.parse_flags(argv, cli.get_config()))
    out = capsys.readouterr().out
    assert math.isfinite(elbo) and math.isfinite(ln_z)
    line = [l for l in out.splitlines() if l.startswith("SMC: ln Z")]
    assert len(line) == 1, out
    r = utils.log_smc_diagnostics.last
    assert math.isfinite(r["smc_ln_Z"]) and math.isfinite(r["smc_ln_Z_std"])
    assert r["smc_stages"] == 3 * len(smc.default_cuts(4)) and 1.0 <= r["smc_ess"] <= 32.0
