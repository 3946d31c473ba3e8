"""Cases, blocks and bars of UHA on lgcp (cmcd_amd.hais_lgcp, cmcd_hais_lgcp.hip), shared by tests/test_oracle_hais_lgcp.py
(CPU: each case is what its row says, and its float32 gap is the stored one) and tests/test_gpu_hais_lgcp.py (the HIP path
against autograd through the float64 restatement, tests/hais_restatement.py on oracle.cmcd_oracle_torch.make_logp_lgcp).

TEST INFRASTRUCTURE ONLY.  A case is `(id, n, K, L, eps, eta, ngrid, sigma, gradient)`.  Parameters:
hais_restatement.make_params(1600, K, L, eps, eta = eta, sigma = sigma, mean_add = mu0, ngrid = ngrid) — a random mean around
mu0 = log 126 - 1.91 / 2 = 3.88, per-dimension logdiag, random md, a non-uniform mgridref_y; seeds synthetic.parity_seeds(n).

What each shape is there for, read against the launch sequence: a call runs one launch per target evaluation on row blocks of
32 particles x column tiles of 16; a block's second 16-row half is computed only when the block has more than 16 rows.

  id          n   K  L  eps    eta  ngrid    why
  n1          1   2  2  0.02   0.6  default  one row
  n16         16  2  2  0.02   0.6  default  the last size without a second 16-row half
  n17         17  2  2  0.02   0.6  default  the first size with one
  n32         32  2  2  0.02   0.6  default  a full row block
  n33         33  2  2  0.02   0.6  default  a one-row second block
  n65         65  2  2  0.02   0.6  default  a third block; slot sums over three blocks
  k1l1        20  1  1  0.02   0.6  default  one bridge, two evaluations, no inner kick; the first boundary is also the last
  l3          20  2  3  0.05   0.6  default  two inner full kicks per bridge
  offgrid     20  3  1  0.02   0.6  5        bridges off the grid's nodes: d / d mgridref_y through the interpolation
  k5grid2     20  5  1  0.1    0.3  2        more bridges than cells
  eta0        20  2  2  0.02   0.0  default  the reference's init_eta; d / d eta at 0
  big         20  3  3  0.2    0.6  default  ten evaluations at a large step (largest eigenvalue of K^-1: 1.57, leap-frog stable)
  refdefault  20  2  1  1e-5   0.0  default  sigma = 1, the reference's default init_eps — FORWARD ONLY: at that step size
                                             d / d md and d / d eta are of order 1e-5 and the restatement's own float32 run
                                             misses them by up to 8e-2 (10 of 83 blocks lost, more than one in ten)

Blocks (`blocks`): vd.mean, vd.logdiag and md per 64 columns (a multiple of the kernel's 16-column tile) and whole; eps and eta
whole; mgridref_y per entry: 82 - 86 blocks per case, each scaled by its own maximum.  A block whose reference is exactly zero
must be exactly zero.

Bars (lgcp_grad_cases' rule): a block is held to BAR = 2e-3 of its own maximum while the restatement's
float32-against-float64 gap on the case's seeds is within a quarter of that, to four times the gap beyond, and is lost beyond
5e-2; at most one block in ten per case may be lost.  The gaps are stored in tests/golden/hais_lgcp_gaps.json (every block of the
twelve gradient cases; loss and z of all thirteen) and re-measured by tests/test_oracle_hais_lgcp.py on at most GAP_THREADS
threads, held to 1.5 x the stored value; a stored value below GAP_FLOOR counts as GAP_FLOOR there, because the last digits of a
float32 product follow the thread count (re-measured on 3 threads the tiny gaps moved by up to 13 x, every one of them still
50 x below the quarter of the bar that decides anything).  Measured: every block's
gap is at most 3.1e-5, so every bar is 2e-3 and no case may lose a block.  No bar comes from what a kernel returned."""
import functools
import json
import math
import os

import numpy as np
import torch

from cmcd_amd import synthetic
from oracle import cmcd_oracle_torch as ot

import hais_restatement as hr
from helpers import lgcp_counts_fixture

D = 1600
MU0 = math.log(126.0) - 0.5 * 1.91
ROW_BLOCK, HALF, COL_TILE = 32, 16, 16          # cmcd_hais_lgcp.hip: kHlRows, the 16-row halves, the column tile

#        id            n   K  L  eps    eta  ngrid sigma gradient
CASES = [("n1",         1, 2, 2, 0.02,  0.6, None, 0.5, True),
         ("n16",       16, 2, 2, 0.02,  0.6, None, 0.5, True),
         ("n17",       17, 2, 2, 0.02,  0.6, None, 0.5, True),
         ("n32",       32, 2, 2, 0.02,  0.6, None, 0.5, True),
         ("n33",       33, 2, 2, 0.02,  0.6, None, 0.5, True),
         ("n65",       65, 2, 2, 0.02,  0.6, None, 0.5, True),
         ("k1l1",      20, 1, 1, 0.02,  0.6, None, 0.5, True),
         ("l3",        20, 2, 3, 0.05,  0.6, None, 0.5, True),
         ("offgrid",   20, 3, 1, 0.02,  0.6, 5,    0.5, True),
         ("k5grid2",   20, 5, 1, 0.1,   0.3, 2,    0.5, True),
         ("eta0",      20, 2, 2, 0.02,  0.0, None, 0.5, True),
         ("big",       20, 3, 3, 0.2,   0.6, None, 0.5, True),
         ("refdefault", 20, 2, 1, 1e-5, 0.0, None, 1.0, False)]
IDS = [c[0] for c in CASES]
GRAD_IDS = [c[0] for c in CASES if c[8]]

BAR = 2e-3              # the suite's standard gradient bar
QUARTER = 0.25          # ... which holds while the restatement's own float32 gap stays within this share of it
FACTOR = 4.0            # otherwise the bar is this multiple of the gap
LOST = 5e-2             # a float32 gap beyond this share of a block's scale: the gradient is no test of that block
MAX_LOST = 0.1          # at most this share of a case's blocks may be lost
GAP_FLOOR = 1e-5        # a stored gap below this is re-measured against 1.5 x this: the last digits follow the summation order
SHARD_TOL = 1e-4        # shards against the single call, of each block's maximum (tests/test_gpu_lgcp_grad.py's)
GAP_THREADS = 8         # the float32 products' summation order follows the thread count (lgcp_grad_cases.run_restatement)
GAPS_PATH = os.path.join(os.path.dirname(__file__), "golden", "hais_lgcp_gaps.json")


def case_by_id(cid):
    return next(c for c in CASES if c[0] == cid)


def seeds_of(case):
    return synthetic.parity_seeds(case[1])


def params(case, device="cpu", trainable=("eta", "eps", "vd", "mgridref_y", "md")):
    """-> (params_flat, unflatten, params_fixed) of the case."""
    _, n, K, L, eps, eta, ngrid, sigma, _ = case
    return hr.make_params(D, K, L, eps, eta=eta, sigma=sigma, mean_add=np.full(D, MU0), ngrid=ngrid, device=device,
                          trainable=trainable)


@functools.lru_cache(maxsize=1)
def logp():
    return ot.make_logp_lgcp(lgcp_counts_fixture())


@functools.lru_cache(maxsize=1)
def target():
    from cmcd_amd.lgcp import load_model_lgcp
    return load_model_lgcp("lgcp", None, flat_bin_counts=lgcp_counts_fixture())[0]


def row_blocks(n):
    """[(rows, has a second 16-row half)] of an n-particle call."""
    sizes = [ROW_BLOCK] * (n // ROW_BLOCK) + ([n % ROW_BLOCK] if n % ROW_BLOCK else [])
    return [(m, m > HALF) for m in sizes]


# ------------------------------------------------------------------------------------------ the restatement
def run_restatement(case, dtype=torch.float64, seeds=None):
    """hais_restatement on the case -> (losses, z, {leaf path: gradient}) as float64 NumPy; the gradient dict is None for a
    forward-only case."""
    flat, un, fixed = params(case)
    p = hr.params_numpy(un, flat)
    seeds = seeds_of(case) if seeds is None else seeds
    threads = torch.get_num_threads()
    if threads > GAP_THREADS:
        torch.set_num_threads(GAP_THREADS)
    try:
        if case[8]:
            l, z, g = hr.bound_and_grad(seeds, p, D, case[2], case[3], logp(), dtype=dtype)
        else:
            (l, z), g = hr.forward(seeds, p, D, case[2], case[3], logp(), dtype=dtype), None
    finally:
        torch.set_num_threads(threads)
    return np.asarray(l, np.float64), np.asarray(z, np.float64), g


@functools.lru_cache(maxsize=None)       # 13 cases x at most 65 x 1600 float64: computed once, shared, read-only
def _reference(cid):
    return run_restatement(case_by_id(cid))


def reference(case):
    return _reference(case[0])


def leaves_of_flat(un, flat):
    """The six differentiable leaves of a flat gradient -> {leaf path: float64 array}."""
    flat = np.asarray(flat, np.float64)
    out = {}
    for path in hr.LEAVES:
        off, shape = un.offset(*path), un.shape(*path)
        size = max(1, int(np.prod(shape)))
        out[path] = flat[off:off + size].reshape(shape)
    return out


# ------------------------------------------------------------------------------------------ blocks
def blocks(g):
    """-> [(name, array)] of a gradient dict: the leaves cut where different code writes them."""
    out = []
    for path in (("vd", "mean"), ("vd", "logdiag"), ("md",)):
        name, a = ".".join(path), np.asarray(g[path], np.float64).reshape(-1)
        out += [("%s[%d:%d]" % (name, c, c + 64), a[c:c + 64]) for c in range(0, D, 64)]
        out.append((name, a))
    for path in (("eps",), ("eta",)):
        out.append((path[0], np.asarray(g[path], np.float64).reshape(-1)))
    my = np.asarray(g[("mgridref_y",)], np.float64).reshape(-1)
    out += [("mgridref_y[%d]" % i, my[i:i + 1]) for i in range(my.size)]
    return out


def block_errors(g, g_ref):
    """-> {block: (max |a - r|, max |r|)}."""
    return {name: (float(np.abs(a - r).max()), float(np.abs(r).max())) for (name, a), (_, r) in zip(blocks(g), blocks(g_ref))}


def worst_particle(l, l_ref):
    return float((np.abs(l - l_ref) / np.maximum(1.0, np.abs(l_ref))).max())


def float32_gap(case):
    """The restatement at float32 against float64 on the case's seeds -> dict(loss = worst loss error over the largest loss,
    z = worst absolute z error, blocks = {block: gap relative to the block's own maximum} for blocks with a non-zero
    reference, zero = [exactly zero ones])."""
    l64, z64, g64 = reference(case)
    l32, z32, g32 = run_restatement(case, dtype=torch.float32)
    assert np.isfinite(l64).all() and np.isfinite(l32).all(), (case[0], "a non-finite reference loss")
    out = dict(loss=float(np.abs(l32 - l64).max() / np.abs(l64).max()), z=float(np.abs(z32 - z64).max()), blocks={}, zero=[])
    if g64 is not None:
        errs = block_errors(g32, g64)
        out["blocks"] = {k: e / s for k, (e, s) in errs.items() if s > 0.0}
        out["zero"] = sorted(k for k, (e, s) in errs.items() if s == 0.0)
    return out


@functools.lru_cache(maxsize=None)
def stored_gaps():
    with open(GAPS_PATH) as f:
        return json.load(f)


def bar_of(gap):
    """The bar of a block whose float32 gap is `gap`: BAR while the gap is within a quarter of it, FACTOR x the gap beyond, None
    (lost) beyond LOST."""
    if gap > LOST:
        return None
    return BAR if gap <= QUARTER * BAR else FACTOR * gap


def compare_blocks(case, g, g_ref, tag=""):
    """Every block of the HIP gradient against the reference under the bars the stored gaps set.
    -> ({block: error / scale}, [failures], [lost blocks])."""
    stored = stored_gaps()[case[0]]["blocks"]
    rep, bad, lost = {}, [], []
    for name, (e, s) in block_errors(g, g_ref).items():
        if s == 0.0:
            if e != 0.0:
                bad.append("%s: expected exactly zero, got up to %.3e" % (name, e))
            continue
        rep[name] = e / s
        bar = bar_of(stored[name])
        if bar is None:
            lost.append(name)
        elif not e <= bar * s:
            bad.append("%s: %.3e of its maximum %.3e (bar %.1e)" % (name, e / s, s, bar))
    return rep, ["%s %s" % (tag, m) for m in bad], lost
