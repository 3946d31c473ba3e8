"""The fused optimiser step on the MI355X (adam_step_kernel of cmcd_amd/csrc/cmcd_opt.hip through cmcd_adam_step and
cmcd_adam_step_dev; vargrad_weights_kernel of cmcd_kernels.hip) against the float64 restatement of the reference's loop body
(tests/opt_restatement.py) on the cases of tests/opt_cases.py.

Bar, per output array: |device - float64 reference| <= max(4 x stored float32 gap, 4 float32 ulps) x max |reference|, the
reference taken from the same float32 inputs, the gap from tests/golden/opt_gaps.json (tests/test_oracle_opt.py keeps it
current).  Where a docstring says "untouched", "unchanged" or "equal", the assertion is on bits."""
import types

import numpy as np
import pytest
import torch

import opt_cases as oc
import opt_restatement as R
from cmcd_amd import _lib, opt

pytestmark = pytest.mark.gpu

WORST = {}       # family -> array -> (observed / max|ref|, bar): printed after the file's last test (-s shows it)


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _state(b):
    return [_dev(b[k]) for k in ("p", "mu", "nu", "ema")]


def _ranges(ranges):
    arr = (_lib.ProjectRange * max(len(ranges), 1))(*[_lib.ProjectRange(o, l, k, 0, lo, hi) for o, l, k, lo, hi in ranges])
    return arr, len(ranges)


def _call(L, st, grad, hyper, ranges, t=None, counter=None, losses=None, diverged=None, stream=None):
    """One step in place on the device tensors st = [p, mu, nu, ema | None]: host form with count `t`, or device-count form
    with the int64 device scalar `counter`."""
    h = dict(R.HYPER)
    h.update(hyper or {})
    arr, cnt = _ranges(ranges)
    ptr = lambda x: None if x is None else x.data_ptr()
    head = (ptr(st[0]), grad.data_ptr(), ptr(st[1]), ptr(st[2]), ptr(st[3]), st[0].numel(), h["lr"], h["b1"], h["b2"], h["eps"],
            h["clip"])
    tail = (h["ema_step"], arr, cnt, ptr(losses), 0 if losses is None else losses.numel(), ptr(diverged), stream)
    if counter is None:
        _lib.check(L.cmcd_adam_step(*head, int(t), *tail))
    else:
        _lib.check(L.cmcd_adam_step_dev(*head, counter.data_ptr(), *tail))


def _host(st):
    torch.cuda.synchronize()
    return tuple(None if a is None else a.cpu().numpy() for a in st)


def _bits(a):
    return a.view(torch.int32) if torch.is_tensor(a) else np.ascontiguousarray(a).view(np.int32)


def _same_bits(xs, ys):
    return all((x is None and y is None) or bool((_bits(x) == _bits(y)).all()) for x, y in zip(xs, ys))


def _within_bar(c, got, want, tag=""):
    dist, bar = oc.distance(got, want), oc.bar(oc.stored_gaps()[c[0]])
    fam = c[3] if c[4][0] == "single" else c[3] + "/trajectory"
    for name in oc.ARRAYS:
        w = WORST.setdefault(fam, {}).get(name, (0.0, 0.0))
        if dist[name] >= w[0]:
            WORST[fam][name] = (dist[name], bar[name])
    bad = {k: (dist[k], bar[k]) for k in oc.ARRAYS if not dist[k] <= bar[k]}
    assert not bad, f"{c[0]} {tag}: (distance, bar) relative to max |reference|: {bad}"
    return dist


@pytest.mark.parametrize("family", oc.FAMILIES)
@pytest.mark.parametrize("n", oc.SIZES)
def test_single_steps_match_optax_in_float64(hip_lib, n, family):
    """Host form, one step with count t from a planted state, every t of the list.  zeros family: an entry with zero gradient
    and zero moments keeps its parameter bits (update exactly 0); one with zero gradient has mu = b1 mu, nu = b2 nu exactly."""
    for c in oc.select(f"single-n{n}-{family}-t"):
        b = oc.build(c)
        st = _state(b)
        _call(hip_lib, st, _dev(b["grad"]), b["hyper"], b["ranges"], t=c[4][1])
        got = _host(st)
        _within_bar(c, got, oc.reference(c, built=b))
        if family == "zeros":
            idx = np.arange(n) % oc.PERIOD if n > oc.PERIOD else np.arange(n)
            dead, zero = idx % 6 == 0, idx % 3 == 0
            assert not b["grad"][zero].any()
            assert np.array_equal(_bits(got[0][dead]), _bits(b["p"][dead])), c[0]
            assert np.array_equal(got[1][zero], np.float32(0.9) * b["mu"][zero]), c[0]
            assert np.array_equal(got[2][zero], np.float32(0.999) * b["nu"][zero]), c[0]
        if family == "nonfinite":
            assert np.isnan(got[0][0]) and np.isnan(got[1][0]) and np.isnan(got[0][n - 1])     # NaN passes the clip ...
            if n >= 6:
                assert np.isfinite(got[0][[1, 2, n - 2, n - 3]]).all()                        # ... +-inf is clipped


@pytest.mark.parametrize("t", oc.STEPS)
def test_device_count_form(hip_lib, t):
    """cmcd_adam_step_dev with *step_counter = t - 1 on the planted states of every size and family: mu and nu equal the host
    form's bits (they do not depend on the count), params and EMA are within the bar (the two forms may differ by the device's
    pow), and the counter reads t afterwards."""
    for n in oc.SIZES:
        for family in oc.FAMILIES:
            c = oc.case(f"single-n{n}-{family}-t{t}")
            b = oc.build(c)
            grad = _dev(b["grad"])
            st_h, st_d = _state(b), _state(b)
            counter = torch.full((1,), t - 1, dtype=torch.int64, device="cuda")
            _call(hip_lib, st_h, grad, b["hyper"], b["ranges"], t=t)
            _call(hip_lib, st_d, grad, b["hyper"], b["ranges"], counter=counter)
            torch.cuda.synchronize()
            assert int(counter) == t, c[0]
            assert _same_bits(st_h[1:3], st_d[1:3]), c[0]
            _within_bar(c, _host(st_d), oc.reference(c, built=b), "device-count form")


def test_device_count_form_counts_a_skipped_step(hip_lib):
    """include/cmcd_hip.h: *step_counter is "incremented by the call" — also by a guarded call whose step is skipped (the
    host form's caller counts such a call too: opt._FusedClipAdam.step).  The four arrays stay untouched."""
    c = oc.case("single-n513-randn-t10")
    b = oc.build(c)
    st, before = _state(b), _state(b)
    counter = torch.full((1,), 9, dtype=torch.int64, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    losses = torch.tensor([1.0, float("nan"), 2.0], device="cuda")
    _call(hip_lib, st, _dev(b["grad"]), b["hyper"], (), counter=counter, losses=losses, diverged=flag)
    torch.cuda.synchronize()
    assert int(counter) == 10 and int(flag) == 1 and _same_bits(st, before)


@pytest.mark.parametrize("cid", [c[0] for c in oc.select("traj-")])
def test_trajectories(hip_lib, cid):
    """T = 200 steps from zero moments, the device fed its own outputs, EMA on: once in host form, once in device-count form
    captured in a graph on a side stream and replayed T times with the gradient copied into a static buffer.  Both within the
    bar of the float64 trajectory at every checked step; mu and nu of the two forms equal in bits."""
    c = oc.case(cid)
    b = oc.build(c)
    want = oc.reference(c, built=b)
    grads = _dev(b["grads"])
    T = c[4][1]
    st_h = _state(b)
    kept = {}
    for k in range(T):
        _call(hip_lib, st_h, grads[b["row"](k)], b["hyper"], b["ranges"], t=k + 1)
        if k + 1 in want:
            got = _host(st_h)
            _within_bar(c, got, want[k + 1], f"host form, step {k + 1}")
            kept[k + 1] = got[1:3]
    st_d = _state(b)
    static_grad = torch.zeros_like(grads[0])
    counter = torch.zeros(1, dtype=torch.int64, device="cuda")
    side = torch.cuda.Stream()
    warm = [torch.zeros(8, device="cuda") for _ in range(4)]            # loads the kernels of this form before the capture
    _call(hip_lib, warm, torch.zeros(8, device="cuda"), {}, (), counter=torch.zeros(1, dtype=torch.int64, device="cuda"))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        _call(hip_lib, st_d, static_grad, b["hyper"], b["ranges"], counter=counter, stream=torch.cuda.current_stream().cuda_stream)
    for k in range(T):
        static_grad.copy_(grads[b["row"](k)])
        graph.replay()
        if k + 1 in want:
            got = _host(st_d)
            _within_bar(c, got, want[k + 1], f"replayed device-count form, step {k + 1}")
            assert _same_bits(got[1:3], kept[k + 1]), (cid, k + 1)
    assert int(counter) == T


@pytest.mark.parametrize("layout", ["b-mcdbm", "b-uha", "b-mfvi", "c"])
def test_projection_ranges(hip_lib, layout):
    """Every entry of every range through every plant (below lo, inside, above hi, NaN, +inf, -inf after the step), and the
    non-finite gradients inside and outside the ranges.  Inside a range: finite values obey it, NaN stays NaN, +-inf go to the
    bound jnp.clip gives; the outside neighbours of every range match the reference WITHOUT projection."""
    for c in oc.select(f"proj-{layout}-") + ([oc.case("hyper-ema0.25-c")] if layout == "c" else []):
        b = oc.build(c)
        st = _state(b)
        _call(hip_lib, st, _dev(b["grad"]), b["hyper"], b["ranges"], t=c[4][1])
        got = _host(st)
        want = oc.reference(c, built=b)
        _within_bar(c, got, want)
        free = oc.reference(c, built=b, ranges=())[0]
        p = got[0].astype(np.float64)
        for r, (off, length, kind, lo, hi) in enumerate(b["ranges"]):
            later = [q for q in b["ranges"][r + 1:] if q[1] > 0]
            pre = R.project(free.copy(), b["ranges"][:r])       # what this range receives: the ranges apply in order
            for i in range(off, off + length):
                if any(o <= i < o + l for o, l, *_ in later):
                    continue                                   # a later range has the last word on this entry
                x = pre[i]
                if np.isnan(x):
                    assert np.isnan(p[i]), (c[0], i)
                elif kind == R.CLAMP:
                    assert lo <= p[i] <= hi, (c[0], i, p[i])
                    if np.isinf(x):
                        assert p[i] == (hi if x > 0 else lo), (c[0], i, p[i])
                else:
                    assert p[i] >= lo and (p[i] == np.inf if x == np.inf else True) and (p[i] == lo if x == -np.inf else True), (c[0], i)
        nb = np.array(oc.neighbours(c))
        fin = np.isfinite(free[nb])                            # (a NaN gradient may sit on a neighbour: NaN both sides)
        assert fin.any() and np.array_equal(np.isnan(p[nb]), np.isnan(free[nb]))
        tol = oc.bar(oc.stored_gaps()[c[0]])["params"] * np.abs(free[np.isfinite(free)]).max()
        assert np.abs(p[nb][fin] - free[nb][fin]).max() <= tol, c[0]
        assert (np.abs(free[nb][fin]) > 6).all()               # still where every projection here would move them


def _guard_losses(n_losses, category, pos):
    """-> (float32 losses, skip expected) or None when n_losses is too small for the category."""
    l = np.random.default_rng(n_losses).standard_normal(n_losses).astype(np.float32) + 3.0
    at = {"0": 0, "255": 255, "256": 256, "last": n_losses - 1}[pos]
    if at >= n_losses:
        return None
    if category == "finite":
        return (l, False) if pos == "0" else None
    if category in ("+inf", "-inf", "nan"):
        l[at] = {"+inf": np.inf, "-inf": -np.inf, "nan": np.nan}[category]
        return l, category == "nan"
    if category == "+inf,-inf@1,258":
        if n_losses < 259 or pos != "0":
            return None
        l[1], l[258] = np.inf, -np.inf
        return l, True
    if category == "nan,+inf":
        if n_losses < 2:
            return None
        l[at], l[(at + 1) % n_losses] = np.nan, np.inf
        return l, True
    if category == "overflow":            # two losses of 3e38: the float32 sum overflows, the mean is +inf, not NaN
        if n_losses < 2 or pos != "0":
            return None
        l[0], l[n_losses - 1] = 3e38, 3e38
        return l, False
    raise KeyError(category)


def test_guard_is_one_decision_for_all_blocks(hip_lib):
    """n = 65 537 parameters: 257 blocks, each scanning the losses for itself (more than one trip of the strided scan from
    n_losses = 257 on).  A skipped step leaves params, mu, nu and ema equal to their bits before in all 257 blocks and the flag
    reads 1; a step that goes through equals the unguarded call in bits and the flag reads 0."""
    c = oc.case("single-n65537-randn-t10")
    b = oc.build(c)
    grad = _dev(b["grad"])
    before = _state(b)
    plain = [a.clone() for a in before]
    _call(hip_lib, plain, grad, b["hyper"], (), t=10)
    torch.cuda.synchronize()
    assert not _same_bits(plain[:1], before[:1])

    def run(losses, flag, guarded=True):
        st = [a.clone() for a in before]
        _call(hip_lib, st, grad, b["hyper"], (), t=10, losses=_dev(losses) if guarded else None, diverged=flag)
        torch.cuda.synchronize()
        return st
    ran = 0
    for n_losses in (1, 3, 256, 257, 1000, 16000):
        for category in ("finite", "+inf", "-inf", "+inf,-inf@1,258", "nan", "nan,+inf", "overflow"):
            for pos in ("0", "255", "256", "last"):
                made = _guard_losses(n_losses, category, pos)
                if made is None:
                    continue
                losses, skip = made
                assert R.mean_is_nan(losses) == skip
                flag = torch.zeros(1, dtype=torch.int32, device="cuda")
                st = run(losses, flag)
                assert int(flag) == int(skip), (n_losses, category, pos)
                assert _same_bits(st, before if skip else plain), (n_losses, category, pos)
                ran += 1
    assert ran >= 80
    finite = _guard_losses(1000, "finite", "0")[0]
    flag = torch.ones(1, dtype=torch.int32, device="cuda")
    assert _same_bits(run(finite, flag), before) and int(flag) == 1                    # a preset flag skips (sticky)
    nan = _guard_losses(1000, "nan", "last")[0]
    assert _same_bits(run(nan, None), before)                                          # no flag to raise: skips all the same
    flag = torch.ones(1, dtype=torch.int32, device="cuda")
    assert _same_bits(run(None, flag, guarded=False), plain) and int(flag) == 1        # no losses: the flag is not consulted


def test_repeated_calls_are_bitwise_identical(hip_lib):
    c = oc.case("single-n65537-randn8-t10")
    b = oc.build(c)
    grad = _dev(b["grad"])
    a, a2 = _state(b), _state(b)
    _call(hip_lib, a, grad, b["hyper"], (), t=10)
    _call(hip_lib, a2, grad, b["hyper"], (), t=10)
    torch.cuda.synchronize()
    assert _same_bits(a, a2)


def test_non_default_stream(hip_lib):
    c = oc.case("single-n65537-randn8-t10")
    b = oc.build(c)
    grad = _dev(b["grad"])
    a, a2 = _state(b), _state(b)
    _call(hip_lib, a, grad, b["hyper"], (), t=10)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        _call(hip_lib, a2, grad, b["hyper"], (), t=10, stream=side.cuda_stream)
    side.synchronize()
    assert _same_bits(a, a2)


def test_hyperparameter_identities(hip_lib):
    """lr = 0: parameter bits unchanged, moments move.  ema_step = 0: EMA bits unchanged.  ema_step = 1: EMA bits equal the
    new parameters.  ema = NULL with ranges: params, mu, nu equal the run with EMA, in bits.  b1 = 0: within the bar."""
    out = {}
    for cid in ("hyper-lr0", "hyper-ema0", "hyper-ema1", "hyper-b10", "hyper-noema-c"):
        c = oc.case(cid)
        b = oc.build(c)
        st = _state(b)
        _call(hip_lib, st, _dev(b["grad"]), b["hyper"], b["ranges"], t=c[4][1])
        got = _host(st)
        _within_bar(c, got, oc.reference(c, built=b))
        out[cid] = (b, got)
    b, got = out["hyper-lr0"]
    assert np.array_equal(_bits(got[0]), _bits(b["p"])) and (got[1] != b["mu"]).all() and (got[2] != b["nu"]).all()
    b, got = out["hyper-ema0"]
    assert np.array_equal(_bits(got[3]), _bits(b["ema"])) and (got[0] != b["p"]).all()
    b, got = out["hyper-ema1"]
    assert np.array_equal(_bits(got[3]), _bits(got[0]))
    b, got = out["hyper-noema-c"]
    assert got[3] is None
    st = _state(b)
    st[3] = _dev(b["p"] + np.float32(0.25))
    _call(hip_lib, st, _dev(b["grad"]), b["hyper"], b["ranges"], t=10)
    with_ema = _host(st)
    assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(got[:3], with_ema[:3]))


@pytest.mark.parametrize("use_graph", [False, True])
def test_opt_run_follows_the_restatement(hip_lib, monkeypatch, use_graph):
    """opt.run for 40 iterations with use_ema=True on the b-mcdbm vector, N = 16, with a prescribed grad_and_loss that needs no
    kernel of the library: row seeds[0] % 64 of a fixed table G[64, n] (tensor indexing: capturable), constant loss.  The CPU
    replays the generator for the rows and runs the restatement.  Eager, and with three eager steps, a capture and 37 replays
    (the first replay is step 4): params and EMA within the bar, count 40, non-trainable leaves keep their bits."""
    c = oc.case("run-b-mcdbm")
    b = oc.build(c)
    flat, unflatten, trainable, _ = oc.b_layout("b-mcdbm")
    T = c[4][1]
    want = oc.reference(c, built=b)[T]
    G = _dev(b["grads"])
    loss = torch.full((16,), 2.5, device="cuda")

    def grad_and_loss(seeds, params_flat, *_):
        return G.index_select(0, (seeds[:1] % 64).long()).reshape(-1), (loss, None)
    counts = []
    real_init = opt._FusedClipAdam.init

    def init(self, params):
        counts.append(real_init(self, params))
        return counts[-1]
    p0 = _dev(b["p"])
    monkeypatch.setattr(opt._FusedClipAdam, "init", init)       # keeps a handle on the optimiser state opt.run does not return
    losses, p, ema = opt.run(types.SimpleNamespace(N=c[6]["N"]), 0.05, T, p0, unflatten, None, None, grad_and_loss, trainable,
                             c[6]["seed"], use_ema=True, use_graph=use_graph)
    torch.cuda.synchronize()
    state = counts[-1]
    assert state["count"] == T and len(losses) == T and np.array_equal(_bits(p0.cpu().numpy()), _bits(b["p"]))
    got = (p.cpu().numpy(), state["mu"].cpu().numpy(), state["nu"].cpu().numpy(), ema.cpu().numpy())
    _within_bar(c, got, want, "graph" if use_graph else "eager")
    for path, (off, shape) in unflatten.layout.items():
        if path[0] == 1:
            sl = slice(off, off + max(int(np.prod(shape)), 1))
            assert np.array_equal(_bits(got[0][sl]), _bits(b["p"][sl])), path


@pytest.mark.parametrize("n", [1, 256, 257, 1000])
def test_vargrad_weights_beyond_one_block(hip_lib, n):
    """cmcd_vargrad_weights with n_total = n and n_total = 3 n + 7: the statistics are those of a float64 batch of n_total
    losses of which these are the first n; yardstick -(2 / n_total)(l - mean) in float64, to 4 float32 ulps of the largest
    weight.  At n = 257 the three branches (variance clip active: all zero; variance NaN: all NaN; inside), in both blocks."""
    from oracle import cmcd_oracle as orc

    def weights(batch, n):
        l = torch.from_numpy(batch[:n].astype(np.float32)).cuda()
        stats = torch.tensor(orc.stats5(batch), dtype=torch.float64, device="cuda")
        om = torch.full((n + 8,), 7.0, device="cuda")
        _lib.check(hip_lib.cmcd_vargrad_weights(l.data_ptr(), stats.data_ptr(), n, batch.size, om.data_ptr(), None))
        torch.cuda.synchronize()
        om = om.cpu().numpy()
        assert (om[n:] == 7.0).all()                               # nothing written past n
        return om[:n]
    for n_total in (n, 3 * n + 7):
        batch = (np.random.default_rng(n_total).standard_normal(n_total) * 3.0 + 1.0).astype(np.float32).astype(np.float64)
        want = -(2.0 / n_total) * (batch[:n] - batch.mean())
        got = weights(batch, n)
        tol = 4 * oc.ULP * max(np.abs(want).max(), np.finfo(np.float32).tiny)
        assert np.abs(got - want).max() <= tol, (n, n_total, np.abs(got - want).max(), tol)
        if n == 257:
            big = batch * 2000.0                                   # variance 3.6e7 > 1e7: the clip passes no gradient
            assert np.var(big) > 1e7 and not weights(big, n).any()
            inside = batch * 500.0                                 # variance 2.3e6: inside
            assert 1e5 < np.var(inside) < 1e7
            want = -(2.0 / n_total) * (inside[:n] - inside.mean())
            assert np.abs(weights(inside, n) - want).max() <= 4 * oc.ULP * np.abs(want).max()
            bad = batch.copy()
            bad[n_total - 1] = np.inf                              # an infinite loss anywhere in the batch: variance NaN
            assert np.isnan(weights(bad, n)).all()


@pytest.fixture(scope="module", autouse=True)
def _report_worst_errors():
    """After the file: the worst observed distance per family and output array beside its bar (pytest -s shows it)."""
    yield
    for fam in sorted(WORST):
        print("opt-worst", fam, " ".join(f"{k}={v[0]:.3e}/{v[1]:.3e}" for k, v in sorted(WORST[fam].items())))
