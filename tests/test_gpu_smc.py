"""Resumable chain segments (include/cmcd_hip.h: cmcd_bound_segment) and the SMC driver (cmcd_amd/smc.py) on the GPU, against
the float64 restatement of tests/smc_restatement.py, which tests/test_smc_oracle.py pins on the CPU.  The reference has no
such call.  Parity goes through helpers.compare_losses / check_stats unchanged, with -(wpath + lg) in the place of the loss.

Fixed seeds (checked on the CPU by tests/test_smc_oracle.py, float64 restatement):
  * FLOOR_*: many_gmm, init_sigma = 60, seeds 1 .. 512 in 2 groups, K = 8, cuts at every bridge, ess_threshold = 1: 10 particles
    have lg = -inf at the first cut, one ancestor of the first stage has 16 offspring, every stage resamples both groups.
  * UNBIASED_*: gmm with init_sigma = 3, seeds 100001 .. 116384 in 64 groups of 256, K = 8, cuts at every bridge,
    ess_threshold = 0.5: mean_g exp(ln Z_g) = 1.0165, std_g = 0.1289, i.e. |mean - 1| = 1.03 std / sqrt(64) <= 2 std / sqrt(64)."""
import numpy as np
import pytest
import torch

from cmcd_amd import mcdboundingmachine as mcdbm
from cmcd_amd import prng, resample, smc, synthetic
from helpers import check_stats, compare_losses
import smc_restatement as rs

FLOOR_SEEDS = synthetic.parity_seeds(512)
FLOOR_CUTS = list(range(1, 8))
FLOOR_RESAMPLE_SEED = 5
UNBIASED_CONFIG, UNBIASED_OVER = "gmm_n300_k8", dict(init_sigma=3.0)
UNBIASED_GROUPS, UNBIASED_M, UNBIASED_RESAMPLE_SEED = 64, 256, 0


def unbiased_seeds():
    return np.arange(100001, 100001 + UNBIASED_GROUPS * UNBIASED_M, dtype=np.int32)


# --------------------------------------------------------------------------- plumbing
def args_of(b):
    return (b["params_flat"], b["unflatten"], b["params_fixed"], b["target"], b["eps_schedule"], b["grad_clipping"])


def dev_seeds(seeds):
    return torch.from_numpy(np.asarray(seeds, np.int32)).cuda()


def to_device(state):
    """A restatement state, rounded to float32, as the device's state dict."""
    key = np.ascontiguousarray(state["key"], np.uint32).view(np.int32)
    return {"z": torch.from_numpy(np.ascontiguousarray(state["z"], np.float32)).cuda(),
            "wpath": torch.from_numpy(np.ascontiguousarray(state["wpath"], np.float32)).cuda(),
            "key": torch.from_numpy(key).cuda(), "k": state["k"]}


def rounded(state):
    """The same state as the restatement continues from: float32 values in float64 arrays."""
    return dict(state, z=state["z"].astype(np.float32).astype(np.float64), wpath=state["wpath"].astype(np.float32).astype(np.float64))


def key_words(state):
    return state["key"].cpu().numpy().view(np.uint32)


def bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64) if t.is_floating_point() else t


def same_bits(a, b, fields=smc.STATE_FIELDS):
    return all(torch.equal(bits(a[f]), bits(b[f])) for f in fields)


def run_device(b, state, k0, k1):
    out = smc.segment(state, k0, k1, *args_of(b))
    torch.cuda.synchronize()
    return out


# --------------------------------------------------------------------------- 1. parity
# (id, config, overrides, n, dense, (k0, k1)): n of {1, 15, 16, 17, 33}; K of {1, 2, 8} and one K = 64; the segments (0, K), (0, 1),
# (K-1, K), (1, K-1); dds and geffner on 2 / 4 / 9 tiles, funnel on 4; the four modes, the three eps schedules, clipping on and off.
PARITY = [
    ("gmm-w22-cais-k8-n33-whole", "gmm_n300_k8", {}, 33, True, (0, 8)),
    ("gmm-w22-cais-k8-n17-middle", "gmm_n300_k8", {}, 17, False, (1, 7)),
    ("gmm-w22-cais-k1-n1", "gmm_n300_k8", dict(nbridges=1), 1, True, (0, 1)),
    ("gmm-w50-var-clip-k8-n15-last", "gmm_n300_k8", dict(boundmode="MCD_CAIS_var_sn", emb_dim=48, grad_clipping=True), 15, True, (7, 8)),
    ("gmm-w22-ula_sn-k2-n16-last", "gmm_n300_k8", dict(boundmode="MCD_ULA_sn", nbridges=2, init_eps=0.05), 16, True, (1, 2)),
    ("gmm-ula-k8-n17-first", "gmm_n300_k8", dict(boundmode="MCD_ULA"), 17, False, (0, 1)),
    ("gmm-dds-linear-k8-n33-middle", "gmm_n300_k8", dict(nn_arch="dds", eps_schedule="linear"), 33, True, (1, 7)),
    ("funnel-w58-cos-k64-n17-whole", "funnel_n300_k64", {}, 17, True, (0, 64)),
    ("funnel-w58-cos-k8-n16-last", "funnel_n300_k64", dict(nbridges=8), 16, True, (7, 8)),
    ("funnel-dds-linear-clip-k8-n15-whole", "funnel_n300_k64", dict(nn_arch="dds", nbridges=8, eps_schedule="linear",
                                                                  grad_clipping=True), 15, False, (0, 8)),
    ("many_gmm-w132-var-clip-k8-n33-middle", "many_gmm_var_n16000_k256", dict(nbridges=8), 33, True, (1, 7)),
    ("many_gmm-dds-cos-clip-k8-n33-whole", "many_gmm_n2000_k256_dds", dict(nbridges=8), 33, True, (0, 8)),
    ("many_gmm-w132-cais-k2-n17-first", "many_gmm_var_n16000_k256", dict(boundmode="MCD_CAIS_sn", nbridges=2, grad_clipping=False),
     17, False, (0, 1)),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", PARITY, ids=[c[0] for c in PARITY])
def test_parity_with_the_restatement(case):
    tag, name, over, n, dense, (k0, k1) = case
    b = synthetic.build(name, device="cuda", dense=dense, **over)
    run = rs.segment_runner(b)
    seeds = synthetic.parity_seeds(n) + 40
    if k0 == 0:
        start_ref, start_dev = seeds, dev_seeds(seeds)
    else:      # a segment with k0 > 0 starts from the restatement's float32-rounded state
        start_ref = rounded(run(seeds, 0, k0))
        start_dev = to_device(start_ref)
    ref = run(start_ref, k0, k1)
    out = run_device(b, start_dev, k0, k1)
    lg, lg_ref = out["lg"].cpu().numpy(), ref["lg"]
    assert not np.isnan(lg).any() and not (lg == np.inf).any()
    assert np.array_equal(lg == -np.inf, lg_ref == -np.inf), f"{tag}: -inf sets of lg differ"
    assert np.array_equal(key_words(out), ref["key"]), f"{tag}: chain key"
    loss = smc.losses_of(out).cpu().numpy()
    print(tag, "loss[:4]", loss[:4], "ref", rs.losses_of(ref)[:4])
    print(tag, compare_losses(loss, rs.losses_of(ref), out["z"].cpu().numpy(), ref["z"], tag, K=k1 - k0))
    fin = np.isfinite(lg_ref)
    werr = np.abs(out["wpath"].cpu().numpy() - ref["wpath"]) / np.maximum(1.0, np.abs(ref["wpath"]))
    lerr = np.abs(lg[fin] - lg_ref[fin]) / np.maximum(1.0, np.abs(lg_ref[fin]))
    print(tag, "wpath rel", werr.max(), "lg rel", lerr.max() if fin.any() else 0.0)
    bound = 1e-3 if k1 - k0 <= 32 else 0.2            # compare_losses' worst-particle bars, on the two addends
    assert werr.max() <= bound and (not fin.any() or lerr.max() <= bound)
    print(tag, check_stats(out["stats"], smc.losses_of(out), tag))


# --------------------------------------------------------------------------- 2, 3. composition bits and the key
@pytest.fixture(scope="module", params=["gmm-k8", "funnel-k64"])
def whole(request):
    if request.param == "gmm-k8":
        b, n = synthetic.build("gmm_n300_k8", device="cuda", dense=True), 33
    else:
        b, n = synthetic.build("funnel_n300_k64", device="cuda", dense=True), 17
    seeds = synthetic.parity_seeds(n)
    return b, seeds, run_device(b, dev_seeds(seeds), 0, b["params_fixed"][1])


@pytest.mark.gpu
def test_two_segments_give_the_bits_of_one(whole):
    b, seeds, full = whole
    K = b["params_fixed"][1]
    for k in (1, K // 2, K - 1):
        head = run_device(b, dev_seeds(seeds), 0, k)
        assert np.array_equal(key_words(head), prng.chain_keys(seeds, k)[k]), f"key leaving [0, {k})"
        tail = run_device(b, head, k, K)
        assert same_bits(tail, full), f"[0, {k}) + [{k}, {K}) != [0, {K})"
        assert torch.equal(bits(tail["stats"]), bits(full["stats"]))
    assert np.array_equal(key_words(full), prng.chain_keys(seeds, K)[K])


# --------------------------------------------------------------------------- 4. the forward call
@pytest.mark.gpu
@pytest.mark.parametrize("name,over,n", [("gmm_n300_k8", {}, 300), ("many_gmm_n2000_k256_dds", dict(nbridges=8), 512),
                                          ("many_gmm_var_n16000_k256", dict(nbridges=8), 49)])
def test_the_whole_segment_matches_the_forward_call(name, over, n):
    b = synthetic.build(name, device="cuda", dense=True, **over)
    K = b["params_fixed"][1]
    seeds = dev_seeds(synthetic.parity_seeds(n))
    out = run_device(b, seeds, 0, K)
    loss_f, z_f, _ = mcdbm.bound_forward(seeds, b["params_flat"], b["unflatten"], b["params_fixed"], b["target"],
                                         eps_schedule=b["eps_schedule"], grad_clipping=b["grad_clipping"])
    torch.cuda.synchronize()
    loss = smc.losses_of(out)
    assert torch.equal(torch.isinf(loss), torch.isinf(loss_f)) and bool((loss[torch.isinf(loss)] > 0).all())
    print(name, compare_losses(loss.cpu().numpy(), loss_f.cpu().numpy(), out["z"].cpu().numpy(), z_f.cpu().numpy(), name, K=K))
    print(name, check_stats(out["stats"], loss, name))


# --------------------------------------------------------------------------- 5. invariances
@pytest.fixture(scope="module")
def staged():
    """funnel, K = 8, 304 particles in 2 groups: the state at bridge 3 and one stage from it (resample, then bridges [3, 6))."""
    b = synthetic.build("funnel_n300_k64", device="cuda", nbridges=8, dense=True)
    seeds = dev_seeds(synthetic.parity_seeds(304))
    head = run_device(b, seeds, 0, 3)

    def stage(state):
        new, info = smc.resample_stage(state, groups=2, ess_threshold=1.0, seed=11)
        return smc.segment(new, 3, 6, *args_of(b)), info

    out, info = stage(head)
    torch.cuda.synchronize()
    return b, seeds, head, stage, out, info


@pytest.mark.gpu
def test_repeated_calls_give_equal_bits(staged):
    b, seeds, head, stage, out, info = staged
    again = run_device(b, seeds, 0, 3)
    assert same_bits(again, head) and torch.equal(bits(again["stats"]), bits(head["stats"]))
    out2, info2 = stage(head)
    torch.cuda.synchronize()
    assert same_bits(out2, out) and torch.equal(info2["ancestors"], info["ancestors"])


@pytest.mark.gpu
def test_a_particle_does_not_depend_on_its_batch(staged):
    b, seeds, head, _, _, _ = staged
    rows = torch.arange(100, 117, device="cuda")       # 17 rows that straddle two tiles of the large batch
    part = run_device(b, seeds[rows].contiguous(), 0, 3)
    assert all(torch.equal(bits(part[f]), bits(head[f][rows])) for f in smc.STATE_FIELDS)
    sub = {f: head[f][rows].contiguous() for f in ("z", "wpath", "key")}
    cont, full = run_device(b, sub, 3, 8), run_device(b, head, 3, 8)
    assert all(torch.equal(bits(cont[f]), bits(full[f][rows])) for f in smc.STATE_FIELDS)


@pytest.mark.gpu
def test_non_default_stream(staged):
    b, seeds, head, stage, out, _ = staged
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got, _ = stage(head)
    side.synchronize()
    assert same_bits(got, out)


@pytest.mark.gpu
def test_one_stage_is_captured_and_replayed(staged):
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
    for f in smc.STATE_FIELDS:
        captured[f].zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(captured, out)
    assert torch.equal(cinfo["ancestors"], info["ancestors"]) and torch.equal(cinfo["resampled"], info["resampled"])
    assert bool(info["resampled"].all())


# --------------------------------------------------------------------------- 6. the driver, step by step
@pytest.mark.gpu
def test_the_driver_is_segments_and_resampling_stages():
    b = synthetic.build("gmm_n300_k8", device="cuda", dense=True)
    K, groups, m = 8, 3, 48
    seeds = dev_seeds(synthetic.parity_seeds(groups * m))
    cuts, thr, seed = [2, 5, 7], 0.9, 4
    out = smc.smc_bound(seeds, *args_of(b), groups=groups, cuts=cuts, ess_threshold=thr, seed=seed, trace=True)
    # by hand
    state = smc.segment(seeds, 0, cuts[0], *args_of(b))
    acc = np.zeros(groups)
    events = []
    for i, c in enumerate(cuts):
        tr = out["trace"][i]
        assert tr["k"] == c and torch.equal(bits(tr["wpath"]), bits(state["wpath"])) and torch.equal(bits(tr["lg"]), bits(state["lg"]))
        loss = smc.losses_of(state)
        z_res, index, st = resample.resample(loss, state["z"], groups=groups, seed=seed + c)
        trig = (st["ess"] < thr * m) & (st["diverged"] == 0)
        events.append(trig)
        mask = trig.repeat_interleave(m)
        anc = torch.where(mask, index.long(), torch.arange(groups * m, device="cuda"))
        assert torch.equal(tr["ancestors"], anc)
        # the float64 evaluation of the stage's ln Z column on the traced float32 values
        w64 = (tr["wpath"].double() + tr["lg"].double()).cpu().numpy().reshape(groups, m)
        col = np.array([np.log(np.exp(r - r.max()).sum()) + r.max() - np.log(m) for r in w64])
        acc += np.where(trig.cpu().numpy(), col, 0.0)
        state = dict(state, z=state["z"][anc], lg=state["lg"][anc], wpath=torch.where(mask, -state["lg"][anc], state["wpath"]))
        state = smc.segment(state, c, cuts[i + 1] if i + 1 < len(cuts) else K, *args_of(b))
    torch.cuda.synchronize()
    assert torch.equal(out["resampled"], torch.stack(events)) and bool(out["resampled"].any())
    assert torch.equal(bits(out["losses"]), bits(smc.losses_of(state))) and torch.equal(bits(out["z"]), bits(state["z"]))
    last = out["trace"][-1]
    assert last["k"] == K and last["ancestors"] is None
    w64 = (last["wpath"].double() + last["lg"].double()).cpu().numpy().reshape(groups, m)
    want = acc + np.array([np.log(np.exp(r - r.max()).sum()) + r.max() - np.log(m) for r in w64])
    assert np.abs(out["ln_Z"].cpu().numpy() - want).max() <= 1e-9
    assert out["ess"].shape == (len(cuts) + 1, groups) and out["ln_Z"].dtype == torch.float64


@pytest.mark.gpu
def test_without_resampling_the_driver_is_the_single_segment(whole):
    b, seeds, full = whole
    K, n = b["params_fixed"][1], len(seeds)
    out = smc.smc_bound(dev_seeds(seeds), *args_of(b), groups=1, cuts=[1, K // 2, K - 1], ess_threshold=0.0)
    torch.cuda.synchronize()
    assert not bool(out["resampled"].any())
    assert torch.equal(bits(out["losses"]), bits(smc.losses_of(full))) and torch.equal(bits(out["z"]), bits(full["z"]))
    column = resample.importance_stats(smc.losses_of(full), 1)["ln_Z"]
    assert torch.equal(bits(out["ln_Z"]), bits(column))
    default = smc.smc_bound(dev_seeds(seeds), *args_of(b), ess_threshold=0.0)      # the default cuts
    assert default["resampled"].shape[0] == len(smc.default_cuts(K)) and torch.equal(bits(default["losses"]), bits(out["losses"]))


# --------------------------------------------------------------------------- 7. floor particles
@pytest.mark.gpu
def test_floor_particles_are_resampled_away():
    b = synthetic.build("many_gmm_n2000_k256_dds", device="cuda", dense=True, nbridges=8)
    assert b["cfg"]["init_sigma"] == 60.0
    n, groups = len(FLOOR_SEEDS), 2
    out = smc.smc_bound(dev_seeds(FLOOR_SEEDS), *args_of(b), groups=groups, cuts=FLOOR_CUTS, ess_threshold=1.0,
                        seed=FLOOR_RESAMPLE_SEED, trace=True)
    torch.cuda.synchronize()
    first = out["trace"][0]
    n_floor = int((first["lg"] == -np.inf).sum())
    print("lg = -inf at the first cut:", n_floor, "events", out["resampled"].sum(0).tolist(), "ln Z", out["ln_Z"].tolist())
    assert n_floor >= 1
    for t in out["trace"]:
        assert not bool(torch.isnan(t["wpath"]).any()) and not bool(torch.isnan(t["lg"]).any())
    for name in ("ln_Z", "losses", "z", "ess"):
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
@pytest.mark.gpu
def test_exp_ln_z_is_unbiased_on_gmm():
    """gmm is normalised (Z = 1): the mean over 64 independent particle systems of exp(ln Z_g) is 1 within 4 standard errors."""
    b = synthetic.build(UNBIASED_CONFIG, device="cuda", dense=True, **UNBIASED_OVER)
    K = b["params_fixed"][1]
    out = smc.smc_bound(dev_seeds(unbiased_seeds()), *args_of(b), groups=UNBIASED_GROUPS, cuts=list(range(1, K)),
                        ess_threshold=0.5, seed=UNBIASED_RESAMPLE_SEED)
    torch.cuda.synchronize()
    zhat = np.exp(out["ln_Z"].cpu().numpy())
    se = zhat.std(ddof=1) / np.sqrt(UNBIASED_GROUPS)
    print("mean exp(ln Z) %.4f, std %.4f, |mean - 1| = %.2f se, events %d" % (zhat.mean(), zhat.std(ddof=1), abs(zhat.mean() - 1) / se,
                                                                           int(out["resampled"].sum())))
    assert bool(out["resampled"].any())
    assert abs(zhat.mean() - 1.0) <= 4.0 * se


# --------------------------------------------------------------------------- 9. the NaN rule
@pytest.mark.gpu
def test_a_nan_group_is_left_alone_and_reports_nan():
    b = synthetic.build("gmm_n300_k8", device="cuda", dense=True)
    groups, m, K = 3, 32, 8
    seeds = dev_seeds(synthetic.parity_seeds(groups * m))
    head = run_device(b, seeds, 0, 4)
    bad = dict(head, wpath=head["wpath"].clone())
    bad["wpath"][m + 5] = float("nan")                 # group 1

    def rest(state):
        new, info = smc.resample_stage(state, groups=groups, ess_threshold=1.0, seed=2)
        end = smc.segment(new, 4, K, *args_of(b))
        return info, end, resample.importance_stats(smc.losses_of(end), groups)["ln_Z"] + info["ln_Z_increment"]

    info_c, end_c, lnz_c = rest(head)
    info_b, end_b, lnz_b = rest(bad)
    torch.cuda.synchronize()
    assert info_b["resampled"].tolist() == [True, False, True] and info_c["resampled"].tolist() == [True, True, True]
    assert torch.equal(info_b["ancestors"][m:2 * m], torch.arange(m, 2 * m, device="cuda"))
    assert bool(torch.isnan(lnz_b[1])) and bool(torch.isnan(end_b["wpath"][m + 5]))
    others = torch.cat([torch.arange(0, m), torch.arange(2 * m, 3 * m)]).cuda()
    assert all(torch.equal(bits(end_b[f][others]), bits(end_c[f][others])) for f in smc.STATE_FIELDS)
    assert torch.equal(bits(lnz_b[[0, 2]]), bits(lnz_c[[0, 2]]))


# --------------------------------------------------------------------------- refusals that need the Python layer
@pytest.mark.gpu
def test_unsupported_configurations_raise():
    seeds = dev_seeds(synthetic.parity_seeds(32))
    for over in (dict(boundmode="MCD_CAIS_UHA_sn"), dict(emb_dim=200)):
        b = synthetic.build("gmm_n300_k8", device="cuda", **over)
        with pytest.raises(NotImplementedError):
            smc.segment(seeds, 0, 2, *args_of(b))
    b = synthetic.build("gmm_n300_k8", device="cuda")
    for k0, k1 in ((0, 9), (3, 3), (-1, 2)):
        with pytest.raises((ValueError, TypeError)):
            smc.segment(seeds if k0 <= 0 else {}, k0, k1, *args_of(b))
    with pytest.raises(ValueError, match="cuts"):
        smc.smc_bound(seeds, *args_of(b), cuts=[0, 3])
