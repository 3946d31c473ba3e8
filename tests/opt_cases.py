"""Cases of the fused optimiser step (adam_step_kernel of cmcd_amd/csrc/cmcd_opt.hip through cmcd_adam_step and
cmcd_adam_step_dev), shared by tests/test_oracle_opt.py (which asserts on the CPU that each case is what it says and keeps the
float32 gaps of tests/golden/opt_gaps.json current) and tests/test_gpu_opt.py (the HIP path against opt_restatement.step at
float64).

A case is `(id, n, layout, family, steps, hyper, extra)`:
  layout  "none" | "b-mcdbm" | "b-uha" | "b-mfvi" | "c"   (RANGES below)
  family  how the gradient is drawn (`_grad`)
  steps   ("single", t): one step with count t from a planted float32 state (p, mu != 0, nu > 0, ema != p);
          ("traj", T): T steps from zero moments, each fed the outputs of the one before; the gradient of step k is row
          `row(k)` of a pool of TRAJ_POOL (or extra["pool"]) draws of the family
  hyper   overrides of opt_restatement.HYPER
  extra   variant (which plant each range entry receives), ema (False: the call gets ema = NULL); rows = "opt.run": the case
          is a run of opt.run(info.N = N, rng_key_gen = seed) on the layout's own params_flat — row(k) is the first seed of
          iteration k modulo the pool, the seeds replayed from a torch generator as opt.run draws them, and the gradient is
          zero on the non-trainable leaves

What each shape reaches, read against the kernel (one thread per entry, 256 per block, grid (n + 255) / 256):
  n = 1            one live lane
  n = 63, 64       one wave short of / exactly a wavefront
  n = 255, 256     one block short of / exactly full
  n = 257          two blocks, one live lane in the second
  n = 511, 513     two blocks one lane short / three blocks with one live lane in the last
  n = 65 537       257 blocks, one live lane in the last (the guard's 257 independent scans)
  n = 1 048 577    4097 blocks, one live lane in the last; 4 MB per array
Above PERIOD entries a vector without ranges repeats its first PERIOD (a prime, so every block sees another phase of it):
the float64 reference is computed on one period and tiled, the device computes and is compared on all n entries.

Range layouts.  (b): what opt._project_ranges returns for three initialisations (`_b_layout`); their leaves sit at the
head of params_flat.  (c), on n = 513 (three blocks): length 1 at offset 0; length 1 at n - 1; [250, 262) across the edge
255 | 256; [256, 512), exactly block 1 (and overlapping the one before on [256, 262)); a zero-length range; a clamp with
hi = +inf; a clamp and a relu floor over the same span [140, 160), clamp first.  In a "proj" case entry j of every range
starts at plant (j + variant) % 6 of PLANTS — below lo, inside, above hi, NaN, +inf, -inf; the step moves a finite one by
less than the margin, test_oracle_opt.py checks that it lands where planted — so the six variants take every entry through
every plant; both outside neighbours of every range (where no other range covers them) hold -7 or +9, which every
projection here would move.

Gradient families.  randn8: 8 randn, about half the entries beyond the +-5 clip.  randn.  loguniform: |g| log-uniform in
[1e-10, 1e-4], random signs, the planted moments of the same size: sqrt(nu_hat) is far below or around eps = 1e-8, so eps
carries the update.  zeros: exact zeros on every third entry, every sixth with zero moments too (update exactly 0,
parameter bits unchanged; the others' moments decay only).  clipedge: +-5 and the float32 neighbours of +-5 on both sides.
nonfinite: NaN, +inf, -inf at the first three and the last three entries (first and last block); nonfinite-dense: on every
third entry, cycling, so that they fall inside and outside every range.

Planted states avoid cancellation (|p| >= 0.5, mu of the gradient's sign): the bar is relative to an array's largest
magnitude, and at n = 1 a cancelling entry would make it a bar on an ill-conditioned sum.
"""
import functools
import os
import zlib

import numpy as np

import opt_restatement as R

SIZES = (1, 63, 64, 255, 256, 257, 511, 513, 65537, 1048577)
FAMILIES = ("randn8", "randn", "loguniform", "zeros", "clipedge", "nonfinite")
STEPS = (1, 2, 10, 1000, 22000, 10 ** 6, 2 ** 31 + 5)
PERIOD = 4099
BLOCK = 256
TRAJ_T = 200
TRAJ_CHECK = tuple(range(1, 11)) + tuple(range(20, TRAJ_T + 1, 20))
TRAJ_POOL = 16
PLANTS = ("below", "inside", "above", "nan", "+inf", "-inf")
ULP = 2.0 ** -23
ARRAYS = ("params", "mu", "nu", "ema")

_C_N = 513
_F = R.f32
LAYOUT_C = (
    (0, 1, R.CLAMP, _F(0.0), _F(0.99)),
    (_C_N - 1, 1, R.CLAMP, _F(1e-7), _F(0.5)),
    (250, 12, R.CLAMP, _F(0.0), _F(0.99)),
    (256, 256, R.RELU_FLOOR, _F(1e-3), 0.0),
    (100, 0, R.CLAMP, _F(0.0), _F(1.0)),
    (120, 10, R.CLAMP, _F(1e-3), float("inf")),
    (140, 20, R.CLAMP, _F(0.2), _F(0.8)),
    (140, 20, R.RELU_FLOOR, _F(0.5), 0.0),
)
B_INITS = {
    "b-mcdbm": ("mcdbm", dict(dim=2, nbridges=8, eps=0.4, eta=0.9, gamma=0.002, mode="MCD_CAIS_sn", nn_arch="geffner", emb_dim=4),
                ("eps", "eta", "gamma", "mgridref_y")),
    "b-uha": ("mcdbm", dict(dim=2, nbridges=8, mode="MCD_CAIS_UHA_sn", nn_arch="geffner", emb_dim=4), ("eta", "gamma")),
    "b-mfvi": ("bm", dict(dim=2, nbridges=8), ("eta", "eps")),
}


@functools.lru_cache(maxsize=None)
def b_layout(name):
    """-> (params_flat (CPU), unflatten, trainable, ranges as tuples) of one of the initialisations of layout (b)."""
    from cmcd_amd import boundingmachine, mcdboundingmachine, opt
    which, kw, trainable = B_INITS[name]
    init = mcdboundingmachine.initialize if which == "mcdbm" else boundingmachine.initialize
    flat, unflatten, _ = init(trainable=trainable, device="cpu", **kw)
    ranges = tuple((int(r.offset), int(r.length), int(r.kind), float(r.lo), float(r.hi))
                   for r in opt._project_ranges(unflatten, trainable))
    return flat, unflatten, trainable, ranges


def ranges_of(layout):
    if layout == "none":
        return ()
    if layout == "c":
        return LAYOUT_C
    return b_layout(layout)[3]


def size_of(layout):
    return _C_N if layout == "c" else int(b_layout(layout)[0].numel())


def _case(cid, n, layout, family, steps, hyper=None, **extra):
    return (cid, n, layout, family, steps, dict(hyper or {}), extra)


def _cases():
    out = []
    for n in SIZES:
        for fam in FAMILIES:
            for t in STEPS:
                out.append(_case(f"single-n{n}-{fam}-t{t}", n, "none", fam, ("single", t)))
    for layout in ("b-mcdbm", "b-uha", "b-mfvi", "c"):
        for v in range(6):
            out.append(_case(f"proj-{layout}-v{v}", None, layout, "randn", ("single", 10), variant=v))
        out.append(_case(f"proj-{layout}-nonfinite", None, layout, "nonfinite-dense", ("single", 10), variant=1))
    # n = 257 carries the ranges of b-mcdbm (165 entries, all ranges in block 0) on a vector of two blocks
    for fam in ("randn8", "loguniform"):
        out.append(_case(f"traj-n257-{fam}", 257, "b-mcdbm", fam, ("traj", TRAJ_T)))
        out.append(_case(f"traj-n65537-{fam}", 65537, "none", fam, ("traj", TRAJ_T)))
    # what opt.run does in 40 iterations on the b-mcdbm vector itself: see test_opt_run_follows_the_restatement
    out.append(_case("run-b-mcdbm", None, "b-mcdbm", "randn8", ("traj", 40), dict(lr=0.05), pool=64, rows="opt.run", seed=7, N=16))
    out.append(_case("hyper-lr0", 513, "none", "randn", ("single", 10), dict(lr=0.0)))
    out.append(_case("hyper-ema0", 513, "none", "randn", ("single", 10), dict(ema_step=0.0)))
    out.append(_case("hyper-ema1", 513, "none", "randn", ("single", 10), dict(ema_step=1.0)))
    out.append(_case("hyper-b10", 513, "none", "randn", ("single", 10), dict(b1=0.0)))
    out.append(_case("hyper-ema0.25-c", None, "c", "randn", ("single", 10), dict(ema_step=0.25), variant=2))
    out.append(_case("hyper-noema-c", None, "c", "randn", ("single", 10), variant=2, ema=False))
    return [(c[0], c[1] if c[1] is not None else size_of(c[2])) + c[2:] for c in out]


@functools.lru_cache(maxsize=None)
def cases():
    return tuple(_cases())


def case(cid):
    return next(c for c in cases() if c[0] == cid)


def select(prefix):
    return [c for c in cases() if c[0].startswith(prefix)]


def base_len(c):
    """Entries the reference is computed on: one period for a long vector without ranges, else n."""
    return PERIOD if (c[2] == "none" and c[1] > PERIOD) else c[1]


def nonfinite_plants(n, m):
    """{base index: value} of the "nonfinite" family on a vector of n entries with period m: the first three entries and
    the last three (index n - 1 - k is base index (n - 1 - k) % m)."""
    vals = (np.nan, np.inf, -np.inf)
    out = {}
    for k in range(min(3, n)):
        out[k % m] = vals[k]
    for k in range(min(3, n)):
        out.setdefault((n - 1 - k) % m, vals[k])
    return out


def _rng(cid, salt=0):
    return np.random.default_rng([zlib.crc32(cid.encode()), salt])


def _grad(family, rng, m, n):
    idx = np.arange(m)
    if family == "randn8":
        g = 8.0 * rng.standard_normal(m)
    elif family == "loguniform":
        g = np.where(rng.random(m) < 0.5, -1.0, 1.0) * 10.0 ** rng.uniform(-10.0, -4.0, m)
    else:
        g = rng.standard_normal(m)
    g = g.astype(np.float32)
    if family == "zeros":
        g[idx % 3 == 0] = 0.0
    elif family == "clipedge":
        five = np.float32(5.0)
        up, down = np.nextafter(five, np.float32(np.inf)), np.nextafter(five, np.float32(-np.inf))
        edge = np.array([five, -five, up, down, -up, -down], np.float32)
        sel = idx % 12 < 6
        g[sel] = edge[idx[sel] % 12]
    elif family == "nonfinite":
        for k, v in nonfinite_plants(n, m).items():
            g[k] = v
    elif family == "nonfinite-dense":
        vals = np.array([np.nan, np.inf, -np.inf], np.float32)
        sel = idx % 3 == 0
        g[sel] = vals[(idx[sel] // 3) % 3]
    return g


def _plant_value(kind, rng_kind, lo, hi):
    """The parameter planted for PLANTS[kind] in a range (rng_kind = R.CLAMP / R.RELU_FLOOR)."""
    bounded = rng_kind == R.CLAMP and np.isfinite(hi)
    return {"below": lo - 1.0, "inside": 0.5 * (lo + hi) if bounded else lo + 1.0,
            "above": hi + 1.0 if bounded else lo + 50.0, "nan": np.nan, "+inf": np.inf, "-inf": -np.inf}[PLANTS[kind]]


def plant_map(c):
    """{index: plant kind} of a "proj" case (a later range of the list overrides an earlier one on a shared entry)."""
    v = c[6].get("variant")
    out = {}
    if v is None:
        return out
    for off, length, _, _, _ in ranges_of(c[2]):
        for j in range(length):
            out[off + j] = (j + v) % 6
    return out


def neighbours(c):
    """Indices next to a range's first or last entry that no range covers."""
    rs = [r for r in ranges_of(c[2]) if r[1] > 0]
    covered = set()
    for off, length, *_ in rs:
        covered.update(range(off, off + length))
    out = set()
    for off, length, *_ in rs:
        out.update(i for i in (off - 1, off + length) if 0 <= i < c[1] and i not in covered)
    return sorted(out)


def _tile(a, n):
    return a if a.size == n else np.tile(a, -(-n // a.size))[:n].copy()


def build(c, full=True):
    """`full=False` keeps one period only (what the reference is computed on).
    -> dict(p, mu, nu, ema, grad [n] float32 — or grads [TRAJ_POOL, n] and `row(k)` for a trajectory —, ranges, hyper, m).
    ema is None when the case runs with ema = NULL."""
    cid, n, layout, family, steps, hyper, extra = c
    m = base_len(c)
    rng = _rng(cid)
    traj = steps[0] == "traj"
    if traj:
        grads = np.stack([_grad(family, _rng(cid, 1 + k), m, n) for k in range(extra.get("pool", TRAJ_POOL))])
        g = grads[0]
    else:
        g = _grad(family, rng, m, n)
    sign = np.where(np.isfinite(g) & (g != 0), np.sign(g), np.where(rng.random(m) < 0.5, -1.0, 1.0))
    if family == "loguniform":
        s = 10.0 ** rng.uniform(-10.0, -4.0, m)
    else:
        s = {"randn8": 8.0, "clipedge": 5.0}.get(family, 1.0) * np.ones(m)
    p = np.where(rng.random(m) < 0.5, -1.0, 1.0) * (0.5 + 2.0 * np.abs(rng.standard_normal(m)))
    mu = sign * s * (0.05 + 0.5 * np.abs(rng.standard_normal(m)))
    nu = s * s * (0.1 + rng.random(m))
    ema = p + 0.3 * (0.1 + rng.random(m))
    if family == "zeros":
        dead = np.arange(m) % 6 == 0
        mu[dead], nu[dead] = 0.0, 0.0
    if traj:
        mu[:], nu[:] = 0.0, 0.0
        if extra.get("rows") == "opt.run":
            flat, unflatten, _, _ = b_layout(layout)
            p = flat.numpy().astype(np.float64)
            for path, (off, shape) in unflatten.layout.items():
                if path[0] == 1:
                    grads[:, off:off + max(int(np.prod(shape)), 1)] = 0.0
        ema = p.copy()
    ranges = ranges_of(layout)
    if layout != "none" and not traj:
        kinds = plant_map(c)
        by_entry = {}
        for off, length, kind, lo, hi in ranges:
            for j in range(length):
                by_entry[off + j] = (kind, lo, hi)
        for i, k in kinds.items():
            p[i] = _plant_value(k, *by_entry[i])
        for j, i in enumerate(neighbours(c)):
            p[i] = -7.0 if (j + extra.get("variant", 0)) % 2 == 0 else 9.0
    n_out = n if full else m
    f = lambda a: _tile(a.astype(np.float32), n_out)
    out = dict(p=f(p), mu=f(mu), nu=f(nu), ema=f(ema) if extra.get("ema", True) else None, ranges=ranges, hyper=hyper, m=m, n=n_out)
    if traj:
        out["grads"] = np.stack([_tile(r, n_out) for r in grads])
        out["row"] = lambda k: (5 * k + k // TRAJ_POOL) % TRAJ_POOL        # k = 0-based step
        if extra.get("rows") == "opt.run":
            import torch
            T, N = steps[1], extra["N"]
            assert T * N <= 1 << 22                                        # one block of opt.run's seed draw
            seeds = torch.randint(1, 1000000, (T * N,), generator=torch.Generator().manual_seed(extra["seed"]), dtype=torch.int32)
            rows = [int(seeds[k * N]) % grads.shape[0] for k in range(T)]
            out["row"] = lambda k: rows[k]
    else:
        out["grad"] = _tile(g, n_out)
    return out


def _head(b, m):
    return tuple(None if b[k] is None else b[k][:m] for k in ("p", "mu", "nu", "ema"))


def reference(c, dtype=np.float64, built=None, ranges=None, one_minus="float32"):
    """Single step -> (params, mu, nu, ema) [n]; trajectory -> {step: (params, mu, nu, ema)} at TRAJ_CHECK.  `ranges`
    replaces the case's (test_projection_ranges: the same step without projection)."""
    b = built or build(c)
    n, m = b["n"], b["m"]
    rs = b["ranges"] if ranges is None else ranges
    if c[4][0] == "single":
        out = R.step(_head(b, m), b["grad"][:m], b["hyper"], c[4][1], rs, dtype=dtype, one_minus=one_minus)[:4]
        return tuple(None if a is None else _tile(a, n) for a in out)
    state, res = _head(b, m), {}
    for k in range(c[4][1]):
        state = R.step(state, b["grads"][b["row"](k)][:m], b["hyper"], k + 1, rs, dtype=dtype, one_minus=one_minus)[:4]
        if k + 1 in TRAJ_CHECK or k + 1 == c[4][1]:
            res[k + 1] = tuple(_tile(a, n) for a in state)
    return res


def distance(got, want):
    """Per output array: max |got - want| over the entries finite in `want`, divided by the largest finite |want| (1 where
    that is 0); the non-finite entries must agree exactly (NaN with NaN, +inf with +inf, -inf with -inf).  ema = None -> 0."""
    out = {}
    for name, a, w in zip(ARRAYS, got, want):
        if w is None:
            assert a is None
            out[name] = 0.0
            continue
        a, w = np.asarray(a, np.float64), np.asarray(w, np.float64)
        fin = np.isfinite(w)
        assert np.array_equal(np.isnan(a), np.isnan(w)), f"{name}: NaN entries differ at {np.flatnonzero(np.isnan(a) != np.isnan(w))[:8]}"
        assert np.array_equal(a[~fin & ~np.isnan(w)], w[~fin & ~np.isnan(w)]), f"{name}: infinite entries differ"
        if not fin.any():
            out[name] = 0.0
            continue
        scale = float(np.abs(w[fin]).max()) or 1.0
        out[name] = float(np.abs(a[fin] - w[fin]).max()) / scale
    return out


def float32_gap(c):
    """The distance of the float32 run of the restatement from the float64 one (a trajectory: the largest over TRAJ_CHECK)."""
    b = build(c, full=False)
    lo, hi = reference(c, np.float32, b), reference(c, np.float64, b)
    if c[4][0] == "single":
        return distance(lo, hi)
    gaps = [distance(lo[k], hi[k]) for k in sorted(hi)]
    return {name: max(g[name] for g in gaps) for name in ARRAYS}


def bar(stored_gap):
    """Per output array, relative to the largest magnitude of the reference: max(4 x stored float32 gap, 4 float32 ulps)."""
    return {name: max(4.0 * stored_gap[name], 4.0 * ULP) for name in ARRAYS}


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "opt_gaps.json")


@functools.lru_cache(maxsize=None)
def stored_gaps():
    import json
    with open(GOLDEN) as f:
        return json.load(f)


if __name__ == "__main__":     # python tests/opt_cases.py --write: record the gaps anew (review the diff)
    import json
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import math

    def up(v):      # three significant digits, rounded up: a re-measured gap never exceeds its record by rounding alone
        if v == 0.0:
            return 0.0
        q = 10.0 ** (math.floor(math.log10(v)) - 2)
        return float(f"{math.ceil(v / q) * q:.3e}")
    gaps = {c[0]: {k: up(v) for k, v in float32_gap(c).items()} for c in cases()}
    if "--write" in sys.argv:
        with open(GOLDEN, "w") as f:
            json.dump(gaps, f, indent=0, sort_keys=True)
            f.write("\n")
    print(len(gaps), "cases; largest gap", max(max(g.values()) for g in gaps.values()))
