"""The yardstick of the fused optimiser step (tests/opt_restatement.py) and its case table (tests/opt_cases.py), checked on
the CPU: against a hand computation, against the eager CPU path of cmcd_amd.opt, against the recorded float32 gaps that set
the bars of tests/test_gpu_opt.py; what the case table claims about itself; opt._project_ranges against opt.project; the
refusals of the two C entry points (decided on the host: no launch, no device); and the seed draw opt.run relies on."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import opt_cases as oc
import opt_restatement as R
from cmcd_amd import _lib, opt


def test_restatement_matches_a_hand_computation_of_two_steps():
    """Steps 1 and 2 on three entries (as tests/test_opt.py), every constant written out: clip, moments of the clipped
    gradient, bias correction, eps outside the root, EMA."""
    h = dict(lr=0.1, ema_step=0.001)
    lr, b1, b2, eps, s = R.f32(0.1), R.f32(0.9), R.f32(0.999), R.f32(1e-8), R.f32(0.001)
    g = np.array([1.0, -10.0, 0.0])
    gc = np.array([1.0, -5.0, 0.0])
    p0 = np.array([0.5, -0.25, 2.0])
    st = (p0, np.zeros(3), np.zeros(3), p0.copy())
    p1, mu1, nu1, ema1, flag, skipped = R.step(st, g, h, 1)
    mu_w, nu_w = (1 - b1) * gc, (1 - b2) * gc ** 2
    p_w = p0 - lr * (mu_w / (1 - b1)) / (np.sqrt(nu_w / (1 - b2)) + eps)
    ema_w = (1 - s) * p0 + s * p_w
    for got, want in ((p1, p_w), (mu1, mu_w), (nu1, nu_w), (ema1, ema_w)):
        assert np.abs(got - want).max() <= 1e-14
    assert p1[2] == 2.0 and flag == 0 and not skipped                 # zero gradient, zero moments: no update
    assert abs((p1[0] - p0[0]) + lr) <= 1e-8                        # step 1 of Adam is -lr sign(g) up to eps
    g2 = np.array([-2.0, 7.0, 3.0])
    gc2 = np.array([-2.0, 5.0, 3.0])
    p2, mu2, nu2, ema2, _, _ = R.step((p1, mu1, nu1, ema1), g2, h, 2)
    mu_w2, nu_w2 = b1 * mu_w + (1 - b1) * gc2, b2 * nu_w + (1 - b2) * gc2 ** 2
    p_w2 = p_w - lr * (mu_w2 / (1 - b1 ** 2)) / (np.sqrt(nu_w2 / (1 - b2 ** 2)) + eps)
    ema_w2 = (1 - s) * ema_w + s * p_w2
    for got, want in ((p2, p_w2), (mu2, mu_w2), (nu2, nu_w2), (ema2, ema_w2)):
        assert np.abs(got - want).max() <= 1e-14
    # the guard: a NaN mean skips, leaves everything and raises the flag; an overflowing float32 sum does not
    out = R.step((p1, mu1, nu1, ema1), g2, h, 2, losses=[1.0, np.inf, -np.inf])
    assert out[5] and out[4] == 1 and all(np.array_equal(a, b) for a, b in zip(out[:4], (p1, mu1, nu1, ema1)))
    assert not R.step((p1, mu1, nu1, ema1), g2, h, 2, losses=np.float32([3e38, 3e38]))[5]
    assert R.step((p1, mu1, nu1, ema1), g2, h, 2, losses=[1.0], flag=1)[5]


_DOUBLE_BOUNDS = {R.f32(1e-7): 1e-7, R.f32(0.5): 0.5, R.f32(0.0): 0.0, R.f32(0.99): 0.99, R.f32(0.001): 0.001, math.inf: math.inf}


def test_restatement_matches_the_eager_cpu_path_in_float64():
    """opt._ClipAdam.update + opt.project + the EMA line of opt.run, on float64 tensors, layout b-mcdbm, five steps.  That
    path takes lr, b, 1 - b and the projection bounds from Python doubles (1 - 0.9, 0.99, ...), not from the float32 values
    of the C ABI: for this ONE comparison the restatement gets the same constants (one_minus="python")."""
    flat, unflatten, trainable, ranges = oc.b_layout("b-mcdbm")
    ranges = [(o, l, k, _DOUBLE_BOUNDS[lo], _DOUBLE_BOUNDS.get(hi, hi)) for o, l, k, lo, hi in ranges]
    n = flat.numel()
    rng = np.random.default_rng(5)
    p = flat.double().clone()
    p[:12] = torch.tensor([0.7, 1.3, -1.0, -3.0, 0.0005, 2.0, 0.001, 1.0, 1.0, 1.0, 1.0, 0.5], dtype=torch.float64)
    eager = opt._ClipAdam(0.05)
    st = eager.init(p)
    ema = p.clone()
    state = (p.numpy().copy(), np.zeros(n), np.zeros(n), p.numpy().copy())
    for t in range(1, 6):
        g = 8.0 * rng.standard_normal(n)
        upd, st = eager.update(torch.from_numpy(g), st, p)
        p.add_(upd)
        opt.project(p, unflatten, trainable)
        ema.mul_(1 - 0.001).add_(p, alpha=0.001)
        state = R.step(state, g, dict(lr=0.05), t, ranges, one_minus="python")[:4]
        for got, want in zip(state, (p, st["mu"], st["nu"], ema)):
            assert np.abs(got - want.numpy()).max() <= 1e-14 * max(1.0, float(want.abs().max())), t
    assert st["count"] == 5


def test_float32_gaps_are_the_recorded_ones():
    """tests/golden/opt_gaps.json (python tests/opt_cases.py --write) holds, per case and output array, the distance of the
    float32 run of the restatement from the float64 one: the device's bar is max(4 x that, 4 float32 ulps).  Re-measured
    here: within 1.5 x both ways where the record sets the bar (above one ulp), and never above a quarter of the bar."""
    stored = oc.stored_gaps()
    assert set(stored) == {c[0] for c in oc.cases()}
    for c in oc.cases():
        gap, rec = oc.float32_gap(c), stored[c[0]]
        bar = oc.bar(rec)
        for name in oc.ARRAYS:
            assert gap[name] <= bar[name] / 4.0, (c[0], name, gap[name], rec[name])
            if rec[name] > oc.ULP:
                assert rec[name] / 1.5 <= gap[name] <= rec[name] * 1.5, (c[0], name, gap[name], rec[name])


def test_case_table_sizes_and_blocks():
    want = {1: (1, 1), 63: (1, 63), 64: (1, 64), 255: (1, 255), 256: (1, 256), 257: (2, 1), 511: (2, 255), 513: (3, 1),
            65537: (257, 1), 1048577: (4097, 1)}
    assert set(oc.SIZES) == set(want)
    for n, (blocks, live) in want.items():
        assert (n + 255) // 256 == blocks and n - (blocks - 1) * 256 == live
        assert len(oc.select(f"single-n{n}-")) == len(oc.FAMILIES) * len(oc.STEPS)
    assert oc.STEPS == (1, 2, 10, 1000, 22000, 10 ** 6, 2 ** 31 + 5)
    # 1 - b2^t is 1 to float32 from t = 22 000 on, and not yet at t = 1000
    b2 = np.float32(0.999)
    assert np.float32(1) - np.float32(float(b2) ** 22000) == 1 and np.float32(1) - np.float32(float(b2) ** 1000) < 1
    assert oc.PERIOD % 2 == 1 and math.gcd(oc.PERIOD, 256) == 1 and 4 * 1048577 <= 4 * 2 ** 20 + 4
    # layout (c): which ranges touch two blocks; the one that is exactly a block; the zero-length one; hi = +inf; the pair
    touch = [l > 0 and o // 256 != (o + l - 1) // 256 for o, l, *_ in oc.LAYOUT_C]
    assert len(oc.LAYOUT_C) == 8 and touch == [False, False, True, False, False, False, False, False]
    assert oc.LAYOUT_C[3][:2] == (256, 256) and oc.LAYOUT_C[4][1] == 0 and oc.LAYOUT_C[5][4] == math.inf
    assert oc.LAYOUT_C[6][:2] == oc.LAYOUT_C[7][:2] and (oc.LAYOUT_C[6][2], oc.LAYOUT_C[7][2]) == (R.CLAMP, R.RELU_FLOOR)
    assert oc.LAYOUT_C[0][:2] == (0, 1) and oc.LAYOUT_C[1][:2] == (512, 1) and oc.size_of("c") == 513
    for name, want_ranges in (("b-mcdbm", 4), ("b-uha", 2), ("b-mfvi", 2)):
        assert len(oc.ranges_of(name)) == want_ranges
    assert oc.size_of("b-mcdbm") <= 257
    # every range has outside neighbours the projection would move, unless another range or the vector's end is there
    c = oc.case("proj-c-v0")
    assert oc.neighbours(c) == [1, 119, 130, 139, 160, 249]
    b = oc.build(c)
    assert all(b["p"][i] in (-7.0, 9.0) for i in oc.neighbours(c))


def test_gradient_families_are_what_the_header_says():
    shares = []
    for c in oc.cases():
        cid, n, layout, family, steps, hyper, extra = c
        if steps[0] != "single" or n > oc.PERIOD and steps[1] != 10:
            continue
        b = oc.build(c, full=False)
        g, m = b["grad"], b["m"]
        if family == "randn8":
            shares.append((np.abs(g) > 5).mean())
            if n >= 255:
                assert 0.4 <= shares[-1] <= 0.7, (cid, shares[-1])
        elif family == "loguniform":
            a = np.abs(g.astype(np.float64))
            assert a.min() >= 1e-10 * (1 - 1e-6) and a.max() <= 1e-4 * (1 + 1e-6)
            _, _, nu, _ = oc.reference(c, built=b)[:4]
            nu_hat = nu[:m] / (1.0 - R.f32(0.999) ** steps[1])
            if n >= 255:        # eps = 1e-8 is at least 1 % of the denominator on a fifth of the entries or more
                assert (R.f32(1e-8) / (np.sqrt(nu_hat) + R.f32(1e-8)) > 0.01).mean() > 0.2, cid
        elif family == "zeros":
            idx = np.arange(m)
            assert not g[idx % 3 == 0].any() and g[idx % 3 != 0].all()
            assert not b["mu"][idx % 6 == 0].any() and not b["nu"][idx % 6 == 0].any() and b["mu"][idx % 6 == 3].all()
        elif family == "clipedge":
            five = np.float32(5)
            want = {five, -five, np.nextafter(five, np.float32(np.inf)), np.nextafter(five, np.float32(0)),
                    -np.nextafter(five, np.float32(np.inf)), -np.nextafter(five, np.float32(0))}
            assert set(g[: min(m, 12)][:6].tolist()) == {float(x) for x in want} or m < 6
        elif family == "nonfinite":
            full = oc.build(c)["grad"]
            assert np.isnan(full[0]) and np.isnan(full[n - 1])
            if n >= 6:
                assert full[1] == np.inf and full[2] == -np.inf and full[n - 2] == np.inf and full[n - 3] == -np.inf
                assert (n - 1) // 256 == (n + 255) // 256 - 1          # the last plants sit in the last block
        if steps[0] == "single" and family != "zeros" and layout == "none":
            assert b["mu"].all() and (b["nu"] > 0).all() and (b["ema"] != b["p"]).all() and (np.abs(b["p"]) >= 0.5).all()
    assert 0.4 <= float(np.mean(shares)) <= 0.7
    # nonfinite-dense on the range layouts: NaN, +inf and -inf each fall inside and outside a range
    for layout in ("b-mcdbm", "c"):
        c = oc.case(f"proj-{layout}-nonfinite")
        g = oc.build(c)["grad"]
        inside = np.zeros(c[1], bool)
        for o, l, *_ in oc.ranges_of(layout):
            inside[o:o + l] = True
        for sel in (np.isnan(g), g == np.inf, g == -np.inf):
            assert (sel & inside).any() and (sel & ~inside).any(), layout


def test_planted_parameters_land_where_the_header_says():
    """Every entry of every range, over the six variants, is below lo, inside, above hi, NaN, +inf and -inf AFTER the step
    and before the projection (the reference without ranges)."""
    for layout in ("b-mcdbm", "b-uha", "b-mfvi", "c"):
        seen = {}
        for v in range(6):
            c = oc.case(f"proj-{layout}-v{v}")
            free = oc.reference(c, ranges=())[0]
            last = {}
            for o, l, kind, lo, hi in oc.ranges_of(layout):
                for j in range(l):
                    last[o + j] = (kind, lo, hi)
            for i, k in oc.plant_map(c).items():
                kind, lo, hi = last[i]
                x, name = free[i], oc.PLANTS[k]
                bounded = kind == R.CLAMP and math.isfinite(hi)
                ok = {"below": x < lo - 0.5, "inside": lo + 0.2 < x < (hi - 0.2 if bounded else math.inf) and x < lo + 2,
                      "above": x > (hi + 0.5 if bounded else lo + 40), "nan": np.isnan(x), "+inf": x == np.inf,
                      "-inf": x == -np.inf}[name]
                assert ok, (layout, v, i, name, x, lo, hi)
                seen.setdefault(i, set()).add(name)
        assert all(s == set(oc.PLANTS) for s in seen.values()) and seen


@pytest.mark.parametrize("name", ["b-mcdbm", "b-uha", "b-mfvi"])
def test_project_ranges_are_opt_project(name):
    """The records the fused step receives (opt._project_ranges) against the eager projection (opt.project) on flat
    float32 vectors filled with -1, with 2 and with NaN: equal in bits, non-trainable leaves included, and no range covers
    an entry of a non-trainable leaf."""
    flat, unflatten, trainable, ranges = oc.b_layout(name)
    n = flat.numel()
    notrain = np.zeros(n, bool)
    for path, (off, shape) in unflatten.layout.items():
        if path[0] == 1:
            notrain[off:off + max(int(np.prod(shape)), 1)] = True
    assert notrain.any()
    for o, l, *_ in ranges:
        assert l >= 1 and not notrain[o:o + l].any()
    for fill in (-1.0, 2.0, float("nan")):
        x = torch.full((n,), fill, dtype=torch.float32)
        want = opt.project(x.clone(), unflatten, trainable).numpy()
        got = R.project(x.numpy().copy(), ranges, np.float32)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), want.view(np.int32)), (name, fill)
        assert np.array_equal(got[notrain].view(np.int32), x.numpy()[notrain].view(np.int32))
    if name == "b-mcdbm":
        moved = R.project(np.full(n, -1.0, np.float32), ranges, np.float32) != -1.0
        assert moved.sum() == 12


def _buf(n=16):
    return (C.c_float * n)()


def _step_args(form, **kw):
    """Arguments of cmcd_adam_step / cmcd_adam_step_dev on host buffers of 16 floats: valid but for what `kw` replaces (no
    call made with them may pass the checks: each case below is refused before any launch)."""
    a = dict(params=_buf(), grad=_buf(), mu=_buf(), nu=_buf(), ema=None, n=16, step=1, counter=(C.c_int64 * 1)(0),
             ranges=None, n_ranges=0, losses=None, n_losses=0, diverged=None)
    a.update(kw)
    keep = [a[k] for k in ("params", "grad", "mu", "nu", "counter", "ranges", "losses")]        # alive during the call
    ptr = lambda x: None if x is None else C.cast(x, C.c_void_p)
    count = a["step"] if form == "host" else ptr(a["counter"])
    return keep, (ptr(a["params"]), ptr(a["grad"]), ptr(a["mu"]), ptr(a["nu"]), ptr(a["ema"]), a["n"], 0.01, 0.9, 0.999, 1e-8,
                  5.0, count, 0.001, a["ranges"], a["n_ranges"], ptr(a["losses"]), a["n_losses"], ptr(a["diverged"]), None)


def _ranges(*rs):
    return (_lib.ProjectRange * max(len(rs), 1))(*[_lib.ProjectRange(o, l, 0, 0, 0.0, 1.0) for o, l in rs])


REFUSALS = [
    ("n_ranges=-1", dict(n_ranges=-1, ranges=_ranges((0, 1))), "at most 8 projection ranges", "both"),
    ("n_ranges=9", dict(n_ranges=9, ranges=_ranges(*[(0, 1)] * 9)), "at most 8 projection ranges", "both"),
    ("null ranges", dict(n_ranges=1, ranges=None), "at most 8 projection ranges", "both"),
    ("negative offset", dict(n_ranges=2, ranges=_ranges((0, 1), (-1, 2))), "projection range outside params_flat", "both"),
    ("negative length", dict(n_ranges=1, ranges=_ranges((3, -1))), "projection range outside params_flat", "both"),
    ("offset+length=n+1", dict(n_ranges=1, ranges=_ranges((9, 8))), "projection range outside params_flat", "both"),
    ("n=0", dict(n=0), "bad argument", "both"),
    ("step=0", dict(step=0), "bad argument", "host"),
    ("null step_counter", dict(counter=None), "bad argument", "dev"),
    ("losses with n_losses=0", dict(losses=_buf(), n_losses=0), "bad argument", "both"),
]


@pytest.mark.parametrize("what,kw,message,forms", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_adam_step_refusals(hip_lib, what, kw, message, forms):
    """Decided on the host before any launch (adam_launch and the two entry points of cmcd_opt.hip): -1 and the message."""
    for form in ("host", "dev"):
        if forms not in ("both", form):
            continue
        keep, args = _step_args(form, **kw)
        fn = hip_lib.cmcd_adam_step if form == "host" else hip_lib.cmcd_adam_step_dev
        rc = fn(*args)
        assert rc == -1 and message in _lib.last_error(), (what, form, rc, _lib.last_error())
        assert keep[4][0] == 0 if keep[4] is not None else True          # the host-side counter buffer is not touched
        with pytest.raises(ValueError):
            _lib.check(rc)


@pytest.mark.parametrize("n", [16, 300, 16000])
def test_one_seed_draw_of_a_block_equals_a_draw_per_iteration(n):
    """opt.run draws the seeds of a block of iterations with ONE randint(nb * n): the same stream as nb draws of n."""
    nb = 5
    a = torch.randint(1, 1000000, (nb * n,), generator=torch.Generator().manual_seed(11), dtype=torch.int32)
    gen = torch.Generator().manual_seed(11)
    b = torch.cat([torch.randint(1, 1000000, (n,), generator=gen, dtype=torch.int32) for _ in range(nb)])
    assert torch.equal(a, b)


def test_opt_run_seeds_across_a_block_boundary():
    """iters * n > 2^22: opt.run draws two blocks (262 iterations of n = 16 000, then one).  The seeds every iteration
    receives are those of one draw of n per iteration from the same generator (nothing patched; the CPU path)."""
    import types
    n, iters = 16000, 263
    assert (1 << 22) // n == 262 and iters * n > 1 << 22
    flat, unflatten, trainable, _ = oc.b_layout("b-mfvi")
    seen = []

    def grad_and_loss(seeds, params_flat, *_):
        seen.append(seeds.clone())
        return torch.zeros_like(params_flat), (torch.ones(4), None)
    losses, p, ema = opt.run(types.SimpleNamespace(N=n), 0.01, iters, flat, unflatten, None, None, grad_and_loss, trainable, 123)
    assert len(seen) == iters and ema is None and torch.equal(p, opt.project(flat.clone(), unflatten, trainable))
    gen = torch.Generator().manual_seed(123)
    for i, s in enumerate(seen):
        assert s.numel() == n and torch.equal(s, torch.randint(1, 1000000, (n,), generator=gen, dtype=torch.int32)), i


def test_the_known_distance_to_optax_constants():
    """optax keeps 1 - b2 as the Python double 1 - 0.999 rounded to float32; the kernel (and the restatement) form
    1 - float32(0.999), exact in float32.  The ratio is 1.0000128, so away from eps optax's update is the kernel's times
    sqrt(1 / 1.0000128) = 1 - 6.4e-6: inside [1 - 1e-5, 1].  Recorded, not changed."""
    ratio = R.f32(1.0 - 0.999) / (1.0 - R.f32(0.999))
    assert abs(ratio - 1.0000128) < 2e-7
    rng = np.random.default_rng(2)
    g = rng.standard_normal(1000)
    g = g[np.abs(g) > 1e-2]
    p0 = np.zeros(g.size)
    st = (p0, np.zeros(g.size), np.zeros(g.size), None)
    ours = R.step(st, g, {}, 1)[0] - p0
    theirs = R.step(st, g, {}, 1, one_minus="optax")[0] - p0
    factor = theirs / ours
    assert (factor >= 1 - 1e-5).all() and (factor <= 1.0).all()
    assert np.abs(factor - math.sqrt(1.0 / ratio)).max() < 1e-7 and abs(math.sqrt(1.0 / ratio) - (1 - 6.4e-6)) < 1e-7
