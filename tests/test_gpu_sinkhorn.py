"""cmcd_amd.sinkhorn.w2_batched (csrc/cmcd_sinkhorn.hip) against a float64 restatement of the Sinkhorn iteration on the CPU.

`restate` is the loop of `utils.W2_distance` with weights; with uniform weights it equals `W2_distance` exactly (asserted
below).  The kernels sum in another order, so a check whose err lies next to stop_thr could fall on either side in two
correct implementations: every case first asserts, on the CPU, that no check of the restatement has err within
[stop_thr / 4, 4 stop_thr] — the seeds below are chosen so that none has.

Tolerances: iterations and status are equal.  cost <= 1 (M <= 1, the plan has mass 1) and is a sum of n^2 terms: the worst-case
float64 summation bound at the largest n here, 500, is n^2 2^-53 = 3e-11, so |cost - restatement| <= 1e-10 absolute.  err is
compared to 1e-3 relative where the restatement's is >= 1e-18 (below that it is rounding of the residuals themselves)."""
import functools

import numpy as np
import pytest
import torch

from cmcd_amd import sinkhorn, utils

pytestmark = pytest.mark.gpu

REG, CAP, THR = 0.01, 10000, 1e-16
R = sinkhorn.ROWS
COST_TOL = 1e-10


def restate(x, y, a, b, reg, num_iter_max, stop_thr, errs=None):
    """-> cost, iterations carried out, err at the last check (NaN without one); `errs` (a list) receives every check's err."""
    x = torch.as_tensor(x, dtype=torch.float64)
    y = torch.as_tensor(y, dtype=torch.float64)
    n = x.shape[0]
    a = torch.full((n,), 1.0 / n, dtype=torch.float64) if a is None else torch.as_tensor(a, dtype=torch.float64)
    b = torch.full((n,), 1.0 / n, dtype=torch.float64) if b is None else torch.as_tensor(b, dtype=torch.float64)
    M = torch.cdist(x, y) ** 2
    M = M / M.max()
    K = torch.exp(-M / reg)
    u, v = torch.ones_like(a) / n, torch.ones_like(b) / n
    iterations, err = 0, float("nan")
    for it in range(num_iter_max):
        KtU = K.t() @ u
        v = b / KtU
        u = a / (K @ v)
        iterations = it + 1
        if it % 10 == 0:
            err = float(torch.linalg.norm(v * (K.t() @ u) - b) ** 2)
            if errs is not None:
                errs.append(err)
            if err < stop_thr:
                break
    P = u[:, None] * K * v[None, :]
    return float((P * M).sum()), iterations, err


# ------------------------------------------------------------------------------------------------------------ the problems
def gmm_like(rng, n, d):
    """a cloud and a target draw of a few well separated Gaussians (different mixing per side)"""
    k = 4
    means = rng.normal(size=(k, d)) * 4.0
    cx, cy = rng.integers(0, k, n), rng.integers(0, k, n)
    return means[cx] + 0.6 * rng.normal(size=(n, d)), means[cy] + 0.5 * rng.normal(size=(n, d))


def funnel_like(rng, n, d):
    """Neal's funnel (sigma = 3) against a narrower approximation of it: a heavy-tailed cost matrix"""
    def draw(s):
        x0 = s * rng.normal(size=(n, 1))
        return np.concatenate([x0, np.exp(x0 / 2) * rng.normal(size=(n, d - 1))], axis=1) if d > 1 else x0
    return draw(2.0), draw(3.0)


def weights(rng, kind, g, n):
    """a[n] for problem g: None = uniform; "weighted": softmax of wide logits with exact zeros, and all the weight of
    problem 1 (problem 0 of a single-problem batch) on one row"""
    if kind == "uniform":
        return None
    if g == 1 or n == 2:
        w = np.zeros(n)
        w[rng.integers(0, n)] = 1.0
        return w
    w = np.exp(rng.normal(size=n) * 1.5)
    w[rng.random(n) < 0.25] = 0.0
    if not w.any():
        w[0] = 1.0
    return w / w.sum()


@functools.lru_cache(maxsize=None)
def problem(cloud, n, d, kind, g, seed):
    """problem g of the family (cloud, n, d, kind): the same whatever batch it is put in -> (x, y, a | None) as float64 arrays"""
    rng = np.random.default_rng([{"gmm": 1, "funnel": 2}[cloud], n, d, g, seed])
    x, y = (gmm_like if cloud == "gmm" else funnel_like)(rng, n, d)
    # (the evaluation's clouds are float32 samples: keep their values exactly representable there)
    x, y = x.astype(np.float32).astype(np.float64), y.astype(np.float32).astype(np.float64)
    return x, y, weights(rng, kind, g, n)


# The guard admits a problem only if its err crosses [stop_thr / 4, 4 stop_thr] between two checks — a fall of more than 16x
# in 10 iterations, so the converging problems here are the quick ones (11 ... 191 iterations) — or never comes near it (the
# funnel problem that runs into the cap at 10 000).  Few random draws do either: these are the seeds per problem g of every
# family (cloud, n, d, weights) that do, found by running `restate` over seeds 0, 1, 2, ...
SEEDS = {
    ("gmm", 2, 2, "uniform"): (2, 0, 0, 1, 1, 1, 0), ("gmm", 63, 2, "uniform"): (435, 209, 261, 175, 176, 804, 19),
    ("gmm", 64, 2, "uniform"): (476, 217, 63, 127, 257, 474, 169), ("gmm", 65, 2, "uniform"): (226, 323, 31, 64, 51, 86, 247),
    ("gmm", 200, 2, "uniform"): (1596, 368, 465, 520, 226, 466, 0), ("gmm", 2, 2, "weighted"): (0, 0, 0),
    ("gmm", 63, 2, "weighted"): (94, 0, 32), ("gmm", 65, 2, "weighted"): (19, 0, 153), ("gmm", 66, 2, "weighted"): (10, 0, 104),
    ("gmm", 129, 2, "weighted"): (5, 0, 421), ("gmm", 200, 2, "weighted"): (1034, 0, 19),
    ("gmm", 66, 2, "uniform"): (390, 594, 0), ("gmm", 129, 2, "uniform"): (192, 0, 1130),
    ("funnel", 65, 10, "uniform"): (3, 2, 1), ("funnel", 65, 10, "weighted"): (0, 0, 0),
    ("gmm", 33, 1, "uniform"): (46, 2, 1), ("gmm", 33, 65, "uniform"): (18, 26, 64), ("gmm", 33, 65, "weighted"): (23, 0, 0),
    ("gmm", 500, 2, "uniform"): (43, 66),
}
CAP200_SEEDS = (3, 1, 0)        # funnel 65 x 10: far from converged after 200 iterations


def seed_of(cloud, n, d, kind, g):
    return SEEDS[(cloud, n, d, kind)][g]


@functools.lru_cache(maxsize=None)
def reference(cloud, n, d, kind, g, cap=CAP, seed=None):
    """the restatement of one problem, computed once -> (cost, iterations, err, status), after the guard on its checks"""
    seed = seed_of(cloud, n, d, kind, g) if seed is None else seed
    x, y, a = problem(cloud, n, d, kind, g, seed)
    errs = []
    cost, iterations, err = restate(x, y, a, None, REG, cap, THR, errs)
    near = [e for e in errs if THR / 4 <= e <= 4 * THR]
    assert not near, f"a check of the restatement has err {near} next to stop_thr: pick another seed for {(cloud, n, d, kind, g)}"
    status = 0 if errs and errs[-1] < THR else 1
    return cost, iterations, err, status


def batch(cloud, n, d, kind, G, seeds=None, device="cuda"):
    ps = [problem(cloud, n, d, kind, g, seed_of(cloud, n, d, kind, g) if seeds is None else seeds[g]) for g in range(G)]
    x = torch.from_numpy(np.stack([p[0] for p in ps])).to(device)
    y = torch.from_numpy(np.stack([p[1] for p in ps])).to(device)
    a = None
    if kind != "uniform":
        a = torch.from_numpy(np.stack([p[2] for p in ps])).to(device)
    return x, y, a


def bits(t):
    return t.contiguous().view(torch.int64)


def host(res):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items()}


def assert_matches(res, refs):
    for g, (cost, iterations, err, status) in enumerate(refs):
        got = {k: float(res[k][g]) for k in sinkhorn.FIELDS}
        print(f"problem {g}: cost {got['cost']:.17g} vs {cost:.17g} (diff {abs(got['cost'] - cost):.3g}), iterations "
              f"{got['iterations']:.0f} vs {iterations}, err {got['err']:.6g} vs {err:.6g}, status {got['status']:.0f} vs {status}")
        assert got["iterations"] == iterations and got["status"] == status, (g, got, iterations, status)
        assert abs(got["cost"] - cost) <= COST_TOL, (g, got["cost"], cost)
        if status == 0:
            assert got["err"] < THR, (g, got["err"])
        if err >= 1e-18:
            assert abs(got["err"] - err) <= 1e-3 * err, (g, got["err"], err)


# n: 2, around one row tile (R - 1, R, R + 1; R + 1 is the first size with two tiles' partials to add, R + 2 the next), three
# tiles, 200; d = 1, 2, 10, 65; G = 1, 3, 7; and one workload-sized case
CASES = [("gmm", G, n, 2, kind) for G in (1, 3, 7) for n in (2, R - 1, R, R + 1, 200) for kind in ("uniform",)]
CASES += [("gmm", 3, n, 2, "weighted") for n in (2, R - 1, R + 1, R + 2, 2 * R + 1, 200)]
CASES += [("gmm", 3, R + 2, 2, "uniform"), ("gmm", 3, 2 * R + 1, 2, "uniform"),
          ("funnel", 3, 65, 10, "uniform"), ("funnel", 3, 65, 10, "weighted"),
          ("gmm", 3, 33, 1, "uniform"), ("gmm", 3, 33, 65, "uniform"), ("gmm", 3, 33, 65, "weighted"),
          ("gmm", 2, 500, 2, "uniform")]
CASES = list(dict.fromkeys(CASES))
IDS = ["%s-G%d-n%d-d%d-%s" % c for c in CASES]


def test_restatement_with_uniform_weights_is_W2_distance_exactly():
    for fam in (("gmm", 65, 2), ("funnel", 65, 10), ("gmm", 33, 1), ("gmm", 200, 2)):
        x, y, _ = problem(*fam, "uniform", 0, 0)
        cost, iterations, _ = restate(x, y, None, None, REG, CAP, THR)
        assert cost == utils.W2_distance(torch.from_numpy(x), torch.from_numpy(y)), fam
        assert 1 <= iterations <= CAP
    x, y, _ = problem("funnel", 65, 10, "uniform", 0, CAP200_SEEDS[0])      # and stopped early, as the cap case below is
    assert restate(x, y, None, None, REG, 200, THR)[0] == utils.W2_distance(torch.from_numpy(x), torch.from_numpy(y),
                                                                             num_iter_max=200)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_matches_the_restatement(case):
    cloud, G, n, d, kind = case
    refs = [reference(cloud, n, d, kind, g) for g in range(G)]
    x, y, a = batch(cloud, n, d, kind, G)
    res = host(sinkhorn.w2_batched(x, y, a=a, reg=REG, num_iter_max=CAP, stop_thr=THR))
    assert_matches(res, refs)


WEIGHTED_B_SEEDS = (13, 0, 168)      # weights(default_rng([9, g, seed])) on the b side of ("gmm", R + 1, 2, "uniform"): passes the guard


def test_weighted_b_matches_the_restatement():
    x, y, _ = batch("gmm", R + 1, 2, "uniform", 3)
    b = np.stack([weights(np.random.default_rng([9, g, WEIGHTED_B_SEEDS[g]]), "weighted", g, R + 1) for g in range(3)])
    assert (b == 0).any(axis=1).all() and b[1].max() == 1.0          # exact zeros everywhere, one group on a single column
    refs = []
    for g in range(3):
        errs = []
        cost, iterations, err = restate(x[g].cpu(), y[g].cpu(), None, b[g], REG, CAP, THR, errs)
        assert not [e for e in errs if THR / 4 <= e <= 4 * THR]
        refs.append((cost, iterations, err, 0 if errs[-1] < THR else 1))
    res = host(sinkhorn.w2_batched(x, y, a=None, b=torch.from_numpy(b).cuda(), reg=REG, num_iter_max=CAP, stop_thr=THR))
    assert_matches(res, refs)


def test_cap_reached_on_a_funnel_cloud():
    refs = [reference("funnel", 65, 10, "uniform", g, cap=200, seed=CAP200_SEEDS[g]) for g in range(3)]
    assert all(r[1] == 200 and r[3] == 1 and r[2] > 1e-12 for r in refs), refs       # none converges by then
    x, y, _ = batch("funnel", 65, 10, "uniform", 3, seeds=CAP200_SEEDS)
    res = host(sinkhorn.w2_batched(x, y, reg=REG, num_iter_max=200, stop_thr=THR))
    assert_matches(res, refs)
    assert list(res["iterations"]) == [200.0] * 3 and list(res["status"]) == [1.0] * 3


def test_the_same_call_twice_gives_the_same_bits():
    x, y, a = batch("gmm", 200, 2, "weighted", 7, seeds=tuple(range(7)))      # any problems will do here
    first = sinkhorn.w2_batched(x, y, a=a)
    second = sinkhorn.w2_batched(x, y, a=a)
    torch.cuda.synchronize()
    for k in sinkhorn.FIELDS:
        assert torch.equal(bits(first[k]), bits(second[k])), k


@pytest.mark.parametrize("n", [R + 1, 200])
def test_bits_do_not_depend_on_batch_polling_or_split(n):
    x, y, _ = batch("gmm", n, 2, "uniform", 7)
    slow = batch("gmm", n, 2, "uniform", 1, seeds=(0,))                      # one that is not among the quick ones
    x[6], y[6] = slow[0][0], slow[1][0]
    g = 4
    alone = sinkhorn.w2_batched(x[g:g + 1], y[g:g + 1])
    runs = {"batch of 7": sinkhorn.w2_batched(x, y),
            "poll_every 10": sinkhorn.w2_batched(x, y, poll_every=10),
            "poll_every 0": sinkhorn.w2_batched(x, y, poll_every=0),
            "split": sinkhorn.w2_batched(x, y, max_workspace_bytes=1)}
    torch.cuda.synchronize()
    assert float(alone["status"][0]) == 0
    for name, res in runs.items():
        for k in sinkhorn.FIELDS:
            assert torch.equal(bits(alone[k][0:1]), bits(res[k][g:g + 1])), (name, k)
            assert torch.equal(bits(runs["batch of 7"][k]), bits(res[k])), (name, k)


def test_graph_capture_and_replay_of_the_unpolled_form():
    x, y, a = batch("gmm", R + 1, 2, "weighted", 3)
    eager = sinkhorn.w2_batched(x, y, a=a, num_iter_max=50, poll_every=0)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = sinkhorn.w2_batched(x, y, a=a, num_iter_max=50, poll_every=0)
    for t in captured.values():
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for k in sinkhorn.FIELDS:
        assert torch.equal(bits(eager[k]), bits(captured[k])), k
    with pytest.raises(RuntimeError, match="poll_every=0"):
        with torch.cuda.graph(torch.cuda.CUDAGraph()):
            sinkhorn.w2_batched(x, y, num_iter_max=50)


@pytest.mark.parametrize("what", ["nan_coordinate", "all_points_equal", "nan_weight"])
def test_degenerate_problem_is_reported_and_leaves_the_others_alone(what):
    x, y, _ = batch("gmm", R + 1, 2, "uniform", 3)
    clean = sinkhorn.w2_batched(x, y)
    x, y = x.clone(), y.clone()
    a = None
    if what == "nan_coordinate":
        y[1, R, 1] = float("nan")
    elif what == "all_points_equal":
        x[1] = 0.25
        y[1] = 0.25
    else:
        a = torch.full(x.shape[:2], 1.0 / x.shape[1], dtype=torch.float64, device=x.device)
        a[1, 0] = float("nan")
    res = sinkhorn.w2_batched(x, y, a=a)
    torch.cuda.synchronize()
    assert float(res["status"][1]) == sinkhorn.UNSOLVABLE and bool(torch.isnan(res["cost"][1]))
    for g in (0, 2):
        for k in sinkhorn.FIELDS:
            assert torch.equal(bits(clean[k][g:g + 1]), bits(res[k][g:g + 1])), (g, k)
        assert float(res["status"][g]) == 0


def test_refusals_of_the_python_entry_point():
    x, y, _ = batch("gmm", 2, 2, "uniform", 1)
    with pytest.raises(RuntimeError, match="runs on a ROCm device only"):
        sinkhorn.w2_batched(x.cpu(), y.cpu())
    with pytest.raises(ValueError):
        sinkhorn.w2_batched(x[:, :1], y[:, :1])             # n = 1
    with pytest.raises(ValueError):
        sinkhorn.w2_batched(x, y[:, :, :1])


OTHER_SEEDS = (10009, 10018, 10004)   # second target draws for ("gmm", R, 2, "uniform") whose target -> other problem passes the guard
LOSS_SEEDS = (16, 6, 6)               # losses for the same clouds whose softmax(-loss)-weighted problem passes the guard


def eval_clouds():
    """[3 * 64, 2] float32 clouds in the layout of the evaluation: sampler cloud, target draw, second target draw"""
    G, n = 3, R
    ps = [problem("gmm", n, 2, "uniform", g, seed_of("gmm", n, 2, "uniform", g)) for g in range(G)]
    others = [problem("gmm", n, 2, "uniform", g, OTHER_SEEDS[g])[1] for g in range(G)]
    f = lambda arrs: torch.from_numpy(np.concatenate(arrs)).float()
    return G, n, f([p[0] for p in ps]), f([p[1] for p in ps]), f(others)


def test_calculate_W2_distances_on_device_tensors_agrees_with_its_loop():
    G, n, cloud, tgt, other = eval_clouds()
    for g in range(G):                                        # the guard, for both problems of every group
        sl = slice(g * n, (g + 1) * n)
        for x, y in ((cloud[sl], tgt[sl]), (tgt[sl], other[sl])):
            errs = []
            restate(x, y, None, None, REG, CAP, THR, errs)
            assert not [e for e in errs if THR / 4 <= e <= 4 * THR]
    loop = utils.calculate_W2_distances(cloud, tgt, other, n, G, n, batched=False)
    assert loop == utils.calculate_W2_distances(cloud, tgt, other, n, G, n)                  # CPU inputs: the loop
    dev = utils.calculate_W2_distances(cloud.cuda(), tgt.cuda(), other.cuda(), n, G, n)
    assert set(dev) == set(loop) == {"w2_dist", "w2_dist_std", "self_w2_dist", "self_w2_dist_std"}
    for k in loop:
        print(k, dev[k], loop[k])
        assert abs(dev[k] - loop[k]) <= COST_TOL, (k, dev[k], loop[k])
    # a shorter n_sinkhorn takes the first rows of every group, and the prefix lands in the keys
    dev = utils.calculate_W2_distances(cloud.cuda(), tgt.cuda(), other.cuda(), n, G, 40, log_prefix="_ema")
    assert set(dev) == {k + "_ema" for k in loop}
    first = lambda t: t.view(G, n, 2)[:, :40].double().cuda()
    direct = sinkhorn.w2_batched(torch.cat([first(cloud), first(tgt)]), torch.cat([first(tgt), first(other)]))["cost"].cpu().numpy()
    assert dev["w2_dist_ema"] == float(np.mean(direct[:G])) and dev["self_w2_dist_std_ema"] == float(np.std(direct[G:]))


def test_losses_add_the_weighted_metric():
    G, n, cloud, tgt, other = eval_clouds()
    losses = np.stack([np.random.default_rng([5, g, LOSS_SEEDS[g]]).normal(size=n) * 2.0 for g in range(G)]).astype(np.float32)
    for g in range(G):
        losses[g, 3 + g] = np.inf
    losses = torch.from_numpy(losses)
    plain = utils.calculate_W2_distances(cloud.cuda(), tgt.cuda(), other.cuda(), n, G, n)
    dev = utils.calculate_W2_distances(cloud.cuda(), tgt.cuda(), other.cuda(), n, G, n, losses=losses.cuda(),
                                       also={"again": cloud.cuda()}, self_w2=(plain["self_w2_dist"], plain["self_w2_dist_std"]))
    assert set(dev) == set(plain) | {"w2_weighted_dist", "w2_weighted_dist_std", "w2_dist_again", "w2_dist_again_std"}
    for k in plain:
        assert dev[k] == plain[k], k                          # the other sets of the batch change nothing
    assert dev["w2_dist_again"] == plain["w2_dist"] and dev["w2_dist_again_std"] == plain["w2_dist_std"]
    costs = []
    for g in range(G):
        w = torch.softmax(-losses[g].double(), dim=0)
        assert w[3 + g] == 0.0                                # a loss of +inf weighs exactly 0
        errs = []
        costs.append(restate(cloud[g * n:(g + 1) * n], tgt[g * n:(g + 1) * n], w, None, REG, CAP, THR, errs)[0])
        assert not [e for e in errs if THR / 4 <= e <= 4 * THR]
    print(dev["w2_weighted_dist"], float(np.mean(costs)), dev["w2_weighted_dist_std"], float(np.std(costs)))
    assert abs(dev["w2_weighted_dist"] - float(np.mean(costs))) <= COST_TOL
    assert abs(dev["w2_weighted_dist_std"] - float(np.std(costs))) <= COST_TOL
    with pytest.raises(RuntimeError, match="runs on a ROCm device only"):
        utils.calculate_W2_distances(cloud, tgt, other, n, G, n, losses=losses)
