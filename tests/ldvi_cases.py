"""The case table of the LDVI tests: tests/test_ldvi_oracle.py asserts on the CPU what each case is there for and keeps the float32
gaps of tests/golden/ldvi_gaps.json current (python tests/ldvi_cases.py --write); tests/test_gpu_ldvi.py runs the HIP path
against the restatement (tests/ldvi_restatement.py) on the same seeds and parameters, under bars taken from those gaps.

Every case is the dense parameter set (cmcd_amd.synthetic.build(dense=True): biases, per-dimension q scales, a non-uniform
mgridref_y, factor_sn = 0.17) of the 2nd-order mode — the reference builds the same tree for `MCD_U_a-lp-sn` — with the mode
string of params_fixed swapped; the network-free case takes MCD_ULA's tree (no `sn`, gamma present).

Shapes, the smallest at which each mechanism can go wrong:
  gmm-n1 .. gmm-n65   gmm, emb 20 (24 wide: 2 neuron tiles), K = 8: one lane, one full tile, a one-particle tail, three tiles, and
                      17 tiles = a second 4-wave workgroup of the sweep with one live wave
  gmm-k1              one bridge: no interior point, z_1 - z_0 pins the draws
  gmm-k40             40 bridges on the 33-node grid: the grid is coarser than the bridges, so the interpolation and its adjoint
                      matter (fractions inside (0, 1), cells with one and with two bridges)
  funnel              d = 10, emb 48 (68 wide: 5 tiles), K = 4, n = 17
  many-floor          many_gmm, K = 8, under a q wide enough that some end points are floored; seeds from 1 .. 64 by the band guard
  nonet               `MCD_U_a-lp` on gmm, n = 33
Past the edges of those ten (the item kernel runs min(K x tiles, 512) one-wave workgroups, workgroup b walks the items b, b + 512,
.. into one slab; the forward kernel takes 1 wave per workgroup up to 1024 tiles, 4 up to 8192, 8 beyond):
  gmm-slabs           K = 40 (gmm-k40's parameters), n = 208: 13 tiles x 40 = 520 items, slabs 0 .. 7 take two items (the second
                      one of another bridge AND another tile), 504 take one
  gmm-slabs-k33       K = 33, n = 257: 17 tiles (the last with one particle) x 33 = 561 items, no multiple of the tile count; the
                      one-particle tile is the second item of three slabs
  funnel-slabs        d = 10 on 5 neuron tiles, K = 64, n = 129: 9 tiles (the last with one particle) x 64 = 576 items
  gmm-w29 / w44 / w64 emb 29 / 40 / 60, n = 17: the 4-tile instances at 33 wide (one unit in tile 3, tile 4 all padding), 44 wide (a
                      whole padded tile) and 64 wide (exact fit)
  many-w64            many_gmm, emb 60, K = 8: the 4-tile instances on the third target; seeds from 1 .. 40 by the band guard
  funnel-w65 / w80    the funnel's parameters with emb 45 / 60: 5 tiles with one unit in the last; exact fit
  funnel-n1/n16/n65   the funnel case at one lane, one full tile, a second sweep workgroup with one live wave
  many-n33            many_gmm, emb 20, K = 8 at the default sigma: the gradient away from the floor regime; band guard on 1 .. 40
  funnel-nonet,       `MCD_U_a-lp` on the funnel (K = 4, n = 17) and on many_gmm (K = 8, band guard on 1 .. 40): the two
  many-nonet          network-free (trajectory, sweep) instances besides gmm's
  gmm-nw4             K = 1, n = 16 400: 1025 tiles -> 4 waves per forward workgroup, 257 workgroups, the last with one live wave;
                      1025 items: one slab of three, 511 of two
  gmm-nw8             K = 1, n = 131 088: 8193 tiles -> 8 waves per workgroup, 1025 workgroups, the last with one live wave; 16 to
                      17 items per slab
The leaves above are cut once more by tests/grad_blocks.py (`compare_blocks` runs both cuts); gmm-nw4 and gmm-nw8 keep the leaf
comparison alone: a float32 restatement of 16 400 / 131 088 particles is more than the CPU suite has for one record.
"""
import functools
import json
import os
import sys

import numpy as np
import torch

if __name__ == "__main__":      # run as a script: the repository root is not on the path yet (under pytest conftest.py puts it there)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import ldvi_restatement as lr
from cmcd_amd import synthetic

GAPS_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ldvi_gaps.json")
BAR = 2e-3          # the suite's gradient bar, of a block's own maximum (tests/test_gpu_grad.py:_compare)
FACTOR = 4.0        # ... or this multiple of the restatement's own float32 gap on the block, whichever is larger
FLOOR = -1e4        # many_gmm's floor of log p (model_handler.py:279-280)
BAND = 500.0        # no evaluation's log p this close to the floor: float32 moves log p by a few units at most out there (checked
                    # on the CPU: the float32 restatement's log p stays within BAND / 10 of the float64 one on every kept seed)

_GMM = dict(config="gmm_n300_k8", over={}, mode="MCD_U_a-lp-sn")
_FUNNEL = dict(config="funnel_n300_k64", over=dict(nbridges=4, init_eps=0.05, init_gamma=4.0), mode="MCD_U_a-lp-sn", n=17)
# many_gmm at ordinary parameters (the configuration's own sigma): seeds from 1 .. `scan` by the band guard
_MANY = dict(config="many_gmm_n2000_k256_dds", mode="MCD_U_a-lp-sn", n=None, scan=40,
             over=dict(nn_arch="geffner", emb_dim=20, nbridges=8, init_eps=0.05, init_gamma=2.0))
SCAN = 64           # the seeds 1 .. SCAN a band-guarded case selects from, unless the case says `scan`
CASES = {
    **{f"gmm-n{n}": dict(_GMM, n=n) for n in (1, 16, 17, 33, 65)},
    "gmm-k1": dict(_GMM, over=dict(nbridges=1), n=17),
    "gmm-k40": dict(_GMM, over=dict(nbridges=40, init_eps=0.02), n=17),
    "funnel": dict(_FUNNEL),
    "many-floor": dict(config="many_gmm_n2000_k256_dds", mode="MCD_U_a-lp-sn", n=None,
                       over=dict(nn_arch="geffner", emb_dim=20, nbridges=8, init_eps=0.2, init_gamma=2.0, init_sigma=100.0)),
    "nonet": dict(_GMM, mode="MCD_U_a-lp", n=33),
    "gmm-slabs": dict(_GMM, over=dict(nbridges=40, init_eps=0.02), n=208),
    "gmm-slabs-k33": dict(_GMM, over=dict(nbridges=33), n=257),
    "funnel-slabs": dict(_FUNNEL, over=dict(nbridges=64, init_eps=0.01, init_gamma=4.0), n=129),
    **{cid: dict(_GMM, over=dict(emb_dim=e), n=17) for cid, e in (("gmm-w29", 29), ("gmm-w44", 40), ("gmm-w64", 60))},
    "many-w64": dict(_MANY, over=dict(_MANY["over"], emb_dim=60)),
    **{f"funnel-w{20 + e}": dict(_FUNNEL, over=dict(_FUNNEL["over"], emb_dim=e)) for e in (45, 60)},
    **{f"funnel-n{n}": dict(_FUNNEL, n=n) for n in (1, 16, 65)},
    "many-n33": dict(_MANY),
    "funnel-nonet": dict(_FUNNEL, mode="MCD_U_a-lp"),
    "many-nonet": dict(_MANY, mode="MCD_U_a-lp"),
    "gmm-nw4": dict(_GMM, over=dict(nbridges=1), n=16400),
    "gmm-nw8": dict(_GMM, over=dict(nbridges=1), n=131088),
}
SHARED = "gmm-n33"   # the case the bit-identity, shard, subset and training tests run on


def build(case_id, device="cpu"):
    """-> dict(params_flat, unflatten, params_fixed, target, cfg) with the LDVI mode string in params_fixed."""
    c = CASES[case_id]
    b = synthetic.build(c["config"], device=device, dense=True,
                        boundmode="MCD_CAIS_UHA_sn" if c["mode"] == "MCD_U_a-lp-sn" else "MCD_ULA", **c["over"])
    dim, K, _, spec = b["params_fixed"]
    b["params_fixed"] = (dim, K, c["mode"], spec)
    return b


@functools.lru_cache(maxsize=None)
def params_of(case_id):
    b = build(case_id)
    return lr.params_numpy(b["unflatten"], b["params_flat"]), b["params_fixed"], b["cfg"]["model"]


@functools.lru_cache(maxsize=None)
def floor_scan(case_id="many-floor"):
    """A band-guarded case on the seeds 1 .. scan it selects from (64 unless the case says otherwise)
    -> (seeds, losses, log p before the floor at the K + 1 evaluations [K + 1, scan])."""
    p, (dim, K, mode, _), model = params_of(case_id)
    seeds = np.arange(1, CASES[case_id].get("scan", SCAN) + 1, dtype=np.int32)
    trace = {}
    l, _ = lr.forward(seeds, p, dim, K, model, use_sn=mode == "MCD_U_a-lp-sn", trace=trace)
    return seeds, l, np.stack(trace["lp"])


@functools.lru_cache(maxsize=None)
def seeds_of(case_id):
    n = CASES[case_id]["n"]
    if n is not None:
        return np.arange(1, n + 1, dtype=np.int32)
    seeds, _, lp = floor_scan(case_id)
    keep = (np.abs(lp - FLOOR) > BAND).all(0)     # the band guard: no evaluation that float32 could take across the floor
    return seeds[keep]


@functools.lru_cache(maxsize=None)
def reference(case_id):
    """The restatement on the case's seeds, once per case and shared (read-only) -> (losses, z, gradient in params_flat order)."""
    p, (dim, K, mode, _), model = params_of(case_id)
    b = build(case_id)
    l, z, g = lr.bound_and_grad(seeds_of(case_id), p, dim, K, model, use_sn=mode == "MCD_U_a-lp-sn")
    return l, z, lr.flat_grad(b["unflatten"], b["params_flat"].numel(), g)


def float32_gap(case_id):
    """The restatement at float32 against float64 on the case's seeds -> dict(loss = worst-particle error over max(1, |loss|),
    blocks = {block: gap over the block's own maximum} for the blocks with a non-zero reference)."""
    p, (dim, K, mode, _), model = params_of(case_id)
    b = build(case_id)
    l64, _, g64 = reference(case_id)
    l32, _, g = lr.bound_and_grad(seeds_of(case_id), p, dim, K, model, use_sn=mode == "MCD_U_a-lp-sn", dtype=torch.float32)
    g32 = lr.flat_grad(b["unflatten"], b["params_flat"].numel(), g)
    assert np.array_equal(np.isinf(l32), np.isinf(l64)), (case_id, "the float32 restatement floors other particles")
    f = np.isfinite(l64)
    return dict(loss=float((np.abs(l32[f] - l64[f]) / np.maximum(1.0, np.abs(l64[f]))).max()),
                blocks={k: e / s for k, (e, s) in lr.block_errors(b["unflatten"], g32, g64).items() if s > 0.0})


@functools.lru_cache(maxsize=None)
def stored_gaps():
    with open(GAPS_PATH) as f:
        return json.load(f)


def bar_of(case_id, block):
    """The bar of a block, relative to its own maximum: max(BAR, FACTOR x the recorded float32 gap)."""
    return max(BAR, FACTOR * stored_gaps()[case_id]["blocks"].get(block, 0.0))


def compare_blocks(case_id, un, flat, flat_ref, tag=""):
    """Every block of a gradient against the reference under `bar_of`; a block whose reference is exactly zero (eta, the
    leaves of params_notrain) must be exactly zero.  -> {block: error over its maximum}."""
    rep, bad = {}, []
    flat, flat_ref = torch.as_tensor(flat).double().cpu(), torch.as_tensor(flat_ref).double().cpu()
    for name, (e, s) in lr.block_errors(un, flat, flat_ref).items():
        if s == 0.0:
            if e != 0.0:
                bad.append("%s: expected exactly zero, got up to %.3e" % (name, e))
            continue
        rep[name] = e / s
        if not e <= bar_of(case_id, name) * s:
            bad.append("%s: %.3e of its maximum %.3e (bar %.1e)" % (name, e / s, s, bar_of(case_id, name)))
    n_train = min(off for path, (off, _) in un.layout.items() if path[0] == 1)
    if float(flat[n_train:].abs().max()) != 0.0:
        bad.append("a leaf of params_notrain has a gradient")
    print(tag or case_id, {k: "%.1e" % v for k, v in rep.items()})
    # ... and the finer cut of tests/grad_blocks.py (neuron tiles, z / rho / embedding rows of W1, emb rows, single entries of
    # mgridref_y and vd) under its own stored gaps, record "ldvi-<case id>"; gmm-nw4 and gmm-nw8 keep the leaves alone
    import grad_blocks as gb
    if case_id not in gb.LDVI_LEAF_ONLY:
        bad += gb.report_blocks("ldvi-" + case_id, "dense", un, flat, flat_ref, tag=tag)
    assert not bad, f"{tag or case_id}: {bad}"
    return rep


def _round_up(x):
    """x rounded up to two significant digits (the record is an upper bound of what was measured)."""
    if x == 0.0:
        return 0.0
    q = 10.0 ** (np.floor(np.log10(x)) - 1)
    return float(np.ceil(x / q) * q)


if __name__ == "__main__":
    if "--write" in sys.argv:
        out = {}
        for cid in CASES:
            g = float32_gap(cid)
            out[cid] = dict(loss=_round_up(g["loss"]), blocks={k: _round_up(v) for k, v in sorted(g["blocks"].items())})
            print(cid, out[cid])
        with open(GAPS_PATH, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")
