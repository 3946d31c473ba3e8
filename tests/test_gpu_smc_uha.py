"""Resumable segments of 2nd-order CMCD (include/cmcd_hip.h: cmcd_bound_segment_uha) and their SMC driver (cmcd_amd/smc_uha.py) on
the GPU, against the float64 restatement of tests/smc_uha_restatement.py, which tests/test_smc_uha_oracle.py pins on the CPU.  The
reference has no such call.  Mirrors tests/test_gpu_smc.py item for item; parity goes through helpers.compare_losses /
check_stats unchanged, with -(wpath + lg) in the place of the loss.

The many_gmm cases run with init_eps = 0.05: the configurations' own step sizes (1.0 / 0.65) with the default gamma = 10 give
eta = gamma eps > 1, a momentum refresh that multiplies rho by (1 - eta) = -9 per bridge — no chain anybody runs, and no
float32 / float64 comparison survives it.

Fixed seeds (checked on the CPU by tests/test_smc_uha_oracle.py, float64 restatement; the measured values are in its docstring):
  * FLOOR_*: many_gmm dds, init_sigma = 60, init_eps = 0.05, seeds 1 .. 512 in 2 groups, K = 8, cuts at every bridge,
    ess_threshold = 1, resampling seed 5: 10 particles have lg = -inf at the first cut, one ancestor of the first stage has 27
    offspring, every stage resamples both groups, ln Z = (-0.402, 0.762).
  * UNBIASED_*: gmm with init_sigma = 3, init_eps = 0.1, seeds 100001 .. 116384 in 64 groups of 256, K = 8, cuts at every bridge,
    ess_threshold = 0.5: 187 resampling events, mean_g exp(ln Z_g) = 0.9870, std_g = 0.2409, i.e. |mean - 1| = 0.43 std / sqrt(64)
    <= 2 std / sqrt(64)."""
import numpy as np
import pytest
import torch

from cmcd_amd import mcdboundingmachine as mcdbm
from cmcd_amd import resample, smc, smc_uha, synthetic
from helpers import check_stats, compare_losses
import smc_uha_restatement as ru

MODE = "MCD_CAIS_UHA_sn"
FLOOR_CONFIG, FLOOR_OVER = "many_gmm_n2000_k256_dds", dict(nbridges=8, init_eps=0.05)
FLOOR_SEEDS = synthetic.parity_seeds(512)
FLOOR_CUTS = list(range(1, 8))
FLOOR_RESAMPLE_SEED = 5
UNBIASED_CONFIG, UNBIASED_OVER = "gmm_n300_k8", dict(init_sigma=3.0, init_eps=0.1)
UNBIASED_GROUPS, UNBIASED_M, UNBIASED_RESAMPLE_SEED = 64, 256, 0


def unbiased_seeds():
    return np.arange(100001, 100001 + UNBIASED_GROUPS * UNBIASED_M, dtype=np.int32)


# --------------------------------------------------------------------------- plumbing
def build(name, dense=True, **over):
    return synthetic.build(name, device="cuda", dense=dense, **dict(dict(boundmode=MODE), **over))


def args_of(b):
    return (b["params_flat"], b["unflatten"], b["params_fixed"], b["target"], b["eps_schedule"], b["grad_clipping"])


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


def same_bits(a, b, fields=smc_uha.STATE_FIELDS):
    return all(torch.equal(bits(a[f]), bits(b[f])) for f in fields)


def run_device(b, state, k0, k1):
    out = smc_uha.segment(state, k0, k1, *args_of(b))
    torch.cuda.synchronize()
    return out


def test_the_state_carries_the_momentum():
    assert smc_uha.STATE_FIELDS == ("z", "rho", "wpath", "lg", "key")


# --------------------------------------------------------------------------- 1. parity
# (id, config, overrides, n, dense, (k0, k1)): n of {1, 15, 16, 17, 33}; K of {1, 2, 8} and one K = 64; the segments (0, K), (0, 1),
# (K-1, K), (1, K-1); gmm geffner 24 (2 tiles) and 44 (zero-padded to 4 tiles); funnel geffner 32 (2 tiles), 68 (5 tiles) and 120
# (zero-padded to 9 tiles); many_gmm geffner 134 (9 tiles); dds on all three targets.
PARITY = [
    ("gmm-w24-k8-n33-whole", "gmm_n300_k8", {}, 33, True, (0, 8)),
    ("gmm-w24-k8-n17-middle", "gmm_n300_k8", {}, 17, False, (1, 7)),
    ("gmm-w24-k1-n1", "gmm_n300_k8", dict(nbridges=1), 1, True, (0, 1)),
    ("gmm-w44-k8-n15-last", "gmm_n300_k8", dict(emb_dim=40), 15, True, (7, 8)),
    ("gmm-w24-k2-n16-last", "gmm_n300_k8", dict(nbridges=2, init_eps=0.05), 16, True, (1, 2)),
    ("gmm-w44-k8-n17-first", "gmm_n300_k8", dict(emb_dim=40), 17, False, (0, 1)),
    ("gmm-dds-k8-n33-middle", "gmm_n300_k8", dict(nn_arch="dds"), 33, True, (1, 7)),
    ("funnel-w68-k64-n17-whole", "funnel_n300_k64", {}, 17, True, (0, 64)),
    ("funnel-w68-k8-n16-last", "funnel_n300_k64", dict(nbridges=8), 16, True, (7, 8)),
    ("funnel-w120-k8-n33-middle", "funnel_n300_k64", dict(nbridges=8, emb_dim=100), 33, True, (1, 7)),
    ("funnel-w32-k2-n15-whole", "funnel_n300_k64", dict(nbridges=2, emb_dim=12), 15, True, (0, 2)),
    ("funnel-dds-k8-n15-whole", "funnel_n300_k64", dict(nn_arch="dds", nbridges=8), 15, False, (0, 8)),
    ("many_gmm-w134-k8-n33-middle", "many_gmm_var_n16000_k256", dict(nbridges=8, init_eps=0.05), 33, True, (1, 7)),
    ("many_gmm-dds-k8-n33-whole", "many_gmm_n2000_k256_dds", dict(nbridges=8, init_eps=0.05), 33, True, (0, 8)),
    ("many_gmm-w134-k2-n17-first", "many_gmm_var_n16000_k256", dict(nbridges=2, init_eps=0.05), 17, False, (0, 1)),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", PARITY, ids=[c[0] for c in PARITY])
def test_parity_with_the_restatement(case):
    tag, name, over, n, dense, (k0, k1) = case
    b = build(name, dense=dense, **over)
    run = ru.segment_runner(b)
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
    loss = smc_uha.losses_of(out).cpu().numpy()
    print(tag, "loss[:4]", loss[:4], "ref", ru.losses_of(ref)[:4])
    print(tag, compare_losses(loss, ru.losses_of(ref), out["z"].cpu().numpy(), ref["z"], tag, K=k1 - k0))
    fin = np.isfinite(lg_ref)
    werr = np.abs(out["wpath"].cpu().numpy() - ref["wpath"]) / np.maximum(1.0, np.abs(ref["wpath"]))
    lerr = np.abs(lg[fin] - lg_ref[fin]) / np.maximum(1.0, np.abs(lg_ref[fin]))
    print(tag, "wpath rel", werr.max(), "lg rel", lerr.max() if fin.any() else 0.0)
    bound = 1e-3 if k1 - k0 <= 32 else 0.2            # compare_losses' worst-particle bars, on the two addends
    assert werr.max() <= bound and (not fin.any() or lerr.max() <= bound)
    # rho to the bar compare_losses holds z to: p99 within 1e-3 of the scale, and every element for chains of <= 32 bridges
    rho, rho_ref = out["rho"].cpu().numpy().astype(np.float64), ref["rho"]
    f = np.isfinite(ru.losses_of(ref))
    rerr = np.abs(rho - rho_ref)[f]
    r_scale = max(1.0, float(np.quantile(np.abs(rho_ref[f]), 0.99)))
    print(tag, "rho p99", float(np.quantile(rerr, 0.99)), "max", float(rerr.max()), "scale", r_scale)
    assert not np.isnan(rho[f]).any() and np.quantile(rerr, 0.99) <= 1e-3 * r_scale
    if k1 - k0 <= 32:
        assert rerr.max() <= 1e-3 * r_scale
    print(tag, check_stats(out["stats"], smc_uha.losses_of(out), tag))


# --------------------------------------------------------------------------- 2, 3. composition bits and the key
@pytest.fixture(scope="module", params=["gmm-k8", "funnel-k64"])
def whole(request):
    if request.param == "gmm-k8":
        b, n = build("gmm_n300_k8"), 33
    else:
        b, n = build("funnel_n300_k64"), 17
    seeds = synthetic.parity_seeds(n)
    return b, seeds, run_device(b, dev_seeds(seeds), 0, b["params_fixed"][1])


@pytest.mark.gpu
def test_two_segments_give_the_bits_of_one(whole):
    import test_smc_uha_oracle as cpu
    b, seeds, full = whole
    K = b["params_fixed"][1]
    for k in (1, K // 2, K - 1):
        head = run_device(b, dev_seeds(seeds), 0, k)
        assert np.array_equal(key_words(head), cpu.forward_key(seeds, k)), f"key leaving [0, {k})"
        tail = run_device(b, head, k, K)
        assert same_bits(tail, full), f"[0, {k}) + [{k}, {K}) != [0, {K})"
        assert torch.equal(bits(tail["stats"]), bits(full["stats"]))
    assert np.array_equal(key_words(full), cpu.forward_key(seeds, K))


# --------------------------------------------------------------------------- 4. the forward call
@pytest.mark.gpu
@pytest.mark.parametrize("name,over,n", [("gmm_n300_k8", {}, 300), ("funnel_n300_k64", dict(nbridges=8), 49),
                                          ("many_gmm_n2000_k256_dds", dict(nbridges=8, init_eps=0.05), 512),
                                          ("many_gmm_var_n16000_k256", dict(nbridges=8, init_eps=0.05), 49)])
def test_the_whole_segment_matches_the_forward_call(name, over, n, monkeypatch):
    monkeypatch.setattr(mcdbm, "KERNEL_VARIANT", 1)      # the forward call on its wave-per-tile kernel
    b = build(name, **over)
    K = b["params_fixed"][1]
    seeds = dev_seeds(synthetic.parity_seeds(n))
    out = run_device(b, seeds, 0, K)
    loss_f, z_f, _ = mcdbm.bound_forward(seeds, b["params_flat"], b["unflatten"], b["params_fixed"], b["target"],
                                         eps_schedule=b["eps_schedule"], grad_clipping=b["grad_clipping"])
    torch.cuda.synchronize()
    loss = smc_uha.losses_of(out)
    assert torch.equal(torch.isinf(loss), torch.isinf(loss_f)) and bool((loss[torch.isinf(loss)] > 0).all())
    print(name, compare_losses(loss.cpu().numpy(), loss_f.cpu().numpy(), out["z"].cpu().numpy(), z_f.cpu().numpy(), name, K=K))
    print(name, check_stats(out["stats"], loss, name))


# --------------------------------------------------------------------------- 5. invariances
@pytest.fixture(scope="module")
def staged():
    """funnel, K = 8, 304 particles in 2 groups: the state at bridge 3 and one stage from it (resample, then bridges [3, 6))."""
    b = build("funnel_n300_k64", nbridges=8)
    seeds = dev_seeds(synthetic.parity_seeds(304))
    head = run_device(b, seeds, 0, 3)

    def stage(state):
        new, info = smc_uha.resample_stage(state, groups=2, ess_threshold=1.0, seed=11)
        return smc_uha.segment(new, 3, 6, *args_of(b)), info

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
    assert all(torch.equal(bits(part[f]), bits(head[f][rows])) for f in smc_uha.STATE_FIELDS)
    sub = {f: head[f][rows].contiguous() for f in ("z", "rho", "wpath", "key")}
    cont, full = run_device(b, sub, 3, 8), run_device(b, head, 3, 8)
    assert all(torch.equal(bits(cont[f]), bits(full[f][rows])) for f in smc_uha.STATE_FIELDS)


@pytest.mark.gpu
def test_a_stage_moves_rho_with_z_and_leaves_the_input_state_alone(staged):
    b, seeds, head, stage, out, info = staged
    before = {f: head[f].clone() for f in smc_uha.STATE_FIELDS}
    new, info2 = smc_uha.resample_stage(head, groups=2, ess_threshold=1.0, seed=11)
    torch.cuda.synchronize()
    anc = info2["ancestors"]
    assert bool(info2["resampled"].all()) and not torch.equal(anc, torch.arange(304, device="cuda"))
    assert torch.equal(bits(new["z"]), bits(head["z"][anc])) and torch.equal(bits(new["rho"]), bits(head["rho"][anc]))
    assert torch.equal(new["key"], head["key"])                      # keys stay with their slot
    assert torch.equal(bits(new["wpath"]), bits(-head["lg"][anc])) and torch.equal(bits(new["lg"]), bits(head["lg"][anc]))
    assert same_bits(head, before)


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
    for f in smc_uha.STATE_FIELDS:
        captured[f].zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(captured, out)
    assert torch.equal(cinfo["ancestors"], info["ancestors"]) and torch.equal(cinfo["resampled"], info["resampled"])
    assert bool(info["resampled"].all())


# --------------------------------------------------------------------------- 6. the driver, step by step
@pytest.mark.gpu
def test_the_driver_is_segments_and_resampling_stages_as_in_the_restatement():
    """smc_bound against the same steps taken by hand on the device, and stage by stage against the restatement: the restatement's
    driver runs on the same seeds and chooses the same ancestors at every stage (they are decided by float64 sums of float32-close
    weights; for these seeds no threshold falls between the two), so z and rho of the final state followed the same ancestors."""
    b = build("gmm_n300_k8")
    K, groups, m = 8, 3, 48
    host_seeds = synthetic.parity_seeds(groups * m)
    seeds = dev_seeds(host_seeds)
    cuts, thr, seed = [2, 5, 7], 0.9, 4
    out = smc_uha.smc_bound(seeds, *args_of(b), groups=groups, cuts=cuts, ess_threshold=thr, seed=seed, trace=True)
    # by hand
    state = smc_uha.segment(seeds, 0, cuts[0], *args_of(b))
    acc = np.zeros(groups)
    events = []
    for i, c in enumerate(cuts):
        tr = out["trace"][i]
        assert tr["k"] == c and torch.equal(bits(tr["wpath"]), bits(state["wpath"])) and torch.equal(bits(tr["lg"]), bits(state["lg"]))
        loss = smc_uha.losses_of(state)
        _, index, st = resample.resample(loss, state["z"], groups=groups, seed=seed + c)
        trig = (st["ess"] < thr * m) & (st["diverged"] == 0)
        events.append(trig)
        mask = trig.repeat_interleave(m)
        anc = torch.where(mask, index.long(), torch.arange(groups * m, device="cuda"))
        assert torch.equal(tr["ancestors"], anc)
        # the float64 evaluation of the stage's ln Z column on the traced float32 values
        w64 = (tr["wpath"].double() + tr["lg"].double()).cpu().numpy().reshape(groups, m)
        col = np.array([np.log(np.exp(r - r.max()).sum()) + r.max() - np.log(m) for r in w64])
        acc += np.where(trig.cpu().numpy(), col, 0.0)
        state = dict(state, z=state["z"][anc], rho=state["rho"][anc], lg=state["lg"][anc],
                     wpath=torch.where(mask, -state["lg"][anc], state["wpath"]))
        state = smc_uha.segment(state, c, cuts[i + 1] if i + 1 < len(cuts) else K, *args_of(b))
    torch.cuda.synchronize()
    assert torch.equal(out["resampled"], torch.stack(events)) and bool(out["resampled"].any())
    assert torch.equal(bits(out["losses"]), bits(smc_uha.losses_of(state))) and torch.equal(bits(out["z"]), bits(state["z"]))
    assert torch.equal(bits(out["rho"]), bits(state["rho"]))
    last = out["trace"][-1]
    assert last["k"] == K and last["ancestors"] is None
    w64 = (last["wpath"].double() + last["lg"].double()).cpu().numpy().reshape(groups, m)
    want = acc + np.array([np.log(np.exp(r - r.max()).sum()) + r.max() - np.log(m) for r in w64])
    assert np.abs(out["ln_Z"].cpu().numpy() - want).max() <= 1e-9
    assert out["ess"].shape == (len(cuts) + 1, groups) and out["ln_Z"].dtype == torch.float64
    # the restatement's driver on the same seeds
    ref = ru.smc_chain(host_seeds, ru.segment_runner(b), K, groups=groups, cuts=cuts, ess_threshold=thr, seed=seed)
    ess = out["ess"].cpu().numpy()
    print("ess", ess, "ref", ref["ess"], "ln Z", out["ln_Z"].tolist(), "ref", ref["ln_Z"])
    # the first cut is reached without a resampling stage.  compare_losses lets a loss be off by d = 1e-3 max(1, |l|); every weight
    # then moves by a factor within exp(+-d), (sum w)^2 and sum w^2 by exp(+-2 d) each, the ESS by exp(+-4 d)
    l0 = ru.losses_of(ref["arrived"][0])
    d = 1e-3 * max(1.0, float(np.abs(l0[np.isfinite(l0)]).max()))
    assert np.all(np.abs(ess[0] - ref["ess"][0]) <= ref["ess"][0] * (np.exp(4 * d) - 1.0))
    # from there on the two runs are comparable while they chose the same ancestors (a threshold of the systematic scheme can fall
    # between the float32 and the float64 cumulative weights)
    same = np.array_equal(out["resampled"].cpu().numpy(), ref["resampled"]) and \
        all(np.array_equal(out["trace"][i]["ancestors"].cpu().numpy(), ref["ancestors"][i]) for i in range(len(cuts)))
    print("events and ancestors equal at every stage:", same)
    assert same      # (fixed seeds: measured so on the MI355X; a change here means the weights at a cut moved)
    if same:
        compare_losses(out["losses"].cpu().numpy(), ref["losses"], out["z"].cpu().numpy(), ref["z"], "driver", K=K)
        assert np.abs(out["rho"].cpu().numpy() - ref["rho"]).max() <= 1e-3 * max(1.0, float(np.quantile(np.abs(ref["rho"]), 0.99)))
        assert np.abs(out["ln_Z"].cpu().numpy() - ref["ln_Z"]).max() <= 1e-3 * max(1.0, np.abs(ref["ln_Z"]).max())


@pytest.mark.gpu
def test_without_resampling_the_driver_is_the_single_segment(whole):
    b, seeds, full = whole
    K, n = b["params_fixed"][1], len(seeds)
    out = smc_uha.smc_bound(dev_seeds(seeds), *args_of(b), groups=1, cuts=[1, K // 2, K - 1], ess_threshold=0.0)
    torch.cuda.synchronize()
    assert not bool(out["resampled"].any())
    assert torch.equal(bits(out["losses"]), bits(smc_uha.losses_of(full))) and torch.equal(bits(out["z"]), bits(full["z"]))
    assert torch.equal(bits(out["rho"]), bits(full["rho"]))
    column = resample.importance_stats(smc_uha.losses_of(full), 1)["ln_Z"]
    assert torch.equal(bits(out["ln_Z"]), bits(column))
    default = smc_uha.smc_bound(dev_seeds(seeds), *args_of(b), ess_threshold=0.0)      # the default cuts
    assert default["resampled"].shape[0] == len(smc_uha.default_cuts(K)) and torch.equal(bits(default["losses"]), bits(out["losses"]))


# --------------------------------------------------------------------------- 7. floor particles
@pytest.mark.gpu
def test_floor_particles_are_resampled_away():
    b = build(FLOOR_CONFIG, **FLOOR_OVER)
    assert b["cfg"]["init_sigma"] == 60.0
    n, groups = len(FLOOR_SEEDS), 2
    out = smc_uha.smc_bound(dev_seeds(FLOOR_SEEDS), *args_of(b), groups=groups, cuts=FLOOR_CUTS, ess_threshold=1.0,
                            seed=FLOOR_RESAMPLE_SEED, trace=True)
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
@pytest.mark.gpu
def test_exp_ln_z_is_unbiased_on_gmm():
    """gmm is normalised (Z = 1): the mean over 64 independent particle systems of exp(ln Z_g) is 1 within 4 standard errors."""
    b = build(UNBIASED_CONFIG, **UNBIASED_OVER)
    K = b["params_fixed"][1]
    out = smc_uha.smc_bound(dev_seeds(unbiased_seeds()), *args_of(b), groups=UNBIASED_GROUPS, cuts=list(range(1, K)),
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
    b = build("gmm_n300_k8")
    groups, m, K = 3, 32, 8
    seeds = dev_seeds(synthetic.parity_seeds(groups * m))
    head = run_device(b, seeds, 0, 4)
    bad = dict(head, wpath=head["wpath"].clone())
    bad["wpath"][m + 5] = float("nan")                 # group 1

    def rest(state):
        new, info = smc_uha.resample_stage(state, groups=groups, ess_threshold=1.0, seed=2)
        end = smc_uha.segment(new, 4, K, *args_of(b))
        return info, end, resample.importance_stats(smc_uha.losses_of(end), groups)["ln_Z"] + info["ln_Z_increment"]

    info_c, end_c, lnz_c = rest(head)
    info_b, end_b, lnz_b = rest(bad)
    torch.cuda.synchronize()
    assert info_b["resampled"].tolist() == [True, False, True] and info_c["resampled"].tolist() == [True, True, True]
    assert torch.equal(info_b["ancestors"][m:2 * m], torch.arange(m, 2 * m, device="cuda"))
    assert bool(torch.isnan(lnz_b[1])) and bool(torch.isnan(end_b["wpath"][m + 5]))
    others = torch.cat([torch.arange(0, m), torch.arange(2 * m, 3 * m)]).cuda()
    assert all(torch.equal(bits(end_b[f][others]), bits(end_c[f][others])) for f in smc_uha.STATE_FIELDS)
    assert torch.equal(bits(lnz_b[[0, 2]]), bits(lnz_c[[0, 2]]))


# --------------------------------------------------------------------------- refusals that need the Python layer
@pytest.mark.gpu
def test_unsupported_configurations_raise():
    seeds = dev_seeds(synthetic.parity_seeds(32))
    for mode in ("MCD_CAIS_sn", "MCD_CAIS_var_sn", "MCD_ULA", "MCD_ULA_sn"):      # every overdamped mode: cmcd_amd.smc's
        b = synthetic.build("gmm_n300_k8", device="cuda", boundmode=mode)
        with pytest.raises(NotImplementedError):
            smc_uha.segment(seeds, 0, 2, *args_of(b))
    b = build("gmm_n300_k8", dense=False, emb_dim=198)                             # width 2 * 2 + 198 = 202: no instance
    with pytest.raises(NotImplementedError):
        smc_uha.segment(seeds, 0, 2, *args_of(b))
    from helpers import lgcp_counts_fixture
    b = synthetic.build("lgcp_n20_k128", device="cuda", lgcp_counts=lgcp_counts_fixture(), boundmode=MODE, nbridges=2)
    with pytest.raises(NotImplementedError, match="lgcp"):
        smc_uha.segment(seeds, 0, 2, *args_of(b))
    b = build("gmm_n300_k8", dense=False)
    for k0, k1 in ((0, 9), (3, 3), (-1, 2)):
        with pytest.raises((ValueError, TypeError)):
            smc_uha.segment(seeds if k0 <= 0 else {}, k0, k1, *args_of(b))
    head = run_device(b, seeds, 0, 2)
    without = {f: head[f] for f in ("z", "wpath", "key")}                          # an overdamped state: no momentum
    with pytest.raises(TypeError, match="rho"):
        smc_uha.segment(without, 2, 4, *args_of(b))
    with pytest.raises(TypeError, match="rho"):
        smc_uha.resample_stage(dict(without, lg=head["lg"]), groups=1)
    with pytest.raises(ValueError, match="cuts"):
        smc_uha.smc_bound(seeds, *args_of(b), cuts=[0, 3])
    with pytest.raises(NotImplementedError, match="smc_uha"):                      # cmcd_amd.smc still refuses this mode
        smc.segment(seeds, 0, 2, *args_of(b))


# --------------------------------------------------------------------------- the evaluation driver
@pytest.mark.gpu
def test_main_runs_the_smc_evaluation_for_the_2nd_order_mode(capsys):
    """python -m cmcd_amd.main --config.boundmode MCD_CAIS_UHA_sn --config.smc_eval: the SMC line is printed (it used to be skipped
    silently for this mode) and its figures are finite."""
    import math
    from cmcd_amd import main as cli
    from cmcd_amd import utils
    argv = ["--config.model", "gmm", "--config.boundmode", MODE, "--config.N", "16", "--config.nbridges", "4",
            "--config.mfvi_iters", "20", "--config.iters", "20", "--config.n_samples", "32", "--config.n_input_dist_seeds", "3",
            "--config.init_eps", "0.01", "--config.lr", "0.001", "--noconfig.compute_w2", "--config.smc_eval"]
    utils.log_smc_diagnostics.last = {}
    elbo, ln_z = cli.main(cli.parse_flags(argv, cli.get_config()))
    out = capsys.readouterr().out
    assert math.isfinite(elbo) and math.isfinite(ln_z)
    line = [l for l in out.splitlines() if l.startswith("SMC: ln Z")]
    assert len(line) == 1, out
    r = utils.log_smc_diagnostics.last
    assert math.isfinite(r["smc_ln_Z"]) and r["smc_stages"] == 3 * len(smc_uha.default_cuts(4)) and 1.0 <= r["smc_ess"] <= 32.0
