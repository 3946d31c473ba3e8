"""Cases of the d = 1600 gradients (cmcd_lgcp.hip: lgcp_grad, lgcp_uha_grad and the deferred contractions lgcp_tn_gemm_kernel,
lgcp_colsum_kernel, launch_geffner_tails), shared by tests/test_oracle_lgcp_grad.py (which asserts on the CPU, from the
restatement alone, that each case is what it says and that its float32 gap is the stored one) and tests/test_gpu_lgcp_grad.py
(the HIP path against autograd through the float64 restatement).

A case is `(id, mode, n, K, form, overrides)`: form 0 leaves the sequence to the library, 3 pins the split-K sequence whose
sweep recomputes every evaluation on a side stream (mcdboundingmachine.KERNEL_VARIANT); `overrides` go to synthetic.build
("lgcp_n20_k128" on tests/golden/lgcp_bin_counts.npy).  init_eps is 2e-3 (0.02 with init_gamma = 5 in the 2nd-order mode), the
seeds are synthetic.parity_seeds(n), every case runs on both parameter sets of the `param_set` fixture.

What each shape is there for, read against the launch sequences.  A call runs in passes of kMP = 32 particles; a pass of
M <= 16 rows takes the no-split-K GEMM, 17 .. 20 its merged instance (rows 16 .. 19 share a workgroup with rows 0 .. 15),
21 .. 32 the split-K GEMM on the activations the forward kept.

  id        n    K  passes        what it reaches
  n1        1    2  1             a single row, dim3(cbD, 1) grids
  n16       16   2  16            the last unmerged size
  n17       17   2  17            the first merged size (clipping on)
  n20       20   2  20            the configuration's own pass (clipping on; the repeat test's kept case)
  n21       21   1  21            the first split-K size on kept activations; K = 1
  n32       32   2  32            a full pass, nothing ragged
  n33       33   3  32 + 1        a one-row second pass
  n52       52   2  32 + 20       a merged pass behind a split-K pass (clipping on)
  n65       65   2  32 + 32 + 1   a third pass: both `base > 0` clears twice (clipping on)
  n129      129  1  4 x 32 + 1    the forward's four lanes wrap; kept rows of a second lane group
  w1612-21  21   2  21            emb_dim = 12: tIN = 101 with a ragged last tile, IN % 128 != 0; split-K family
  w1612-37  37   2  32 + 5        the same width on both GEMM families
  w1604     20   2  20            emb_dim = 4
  w1670-5   5    2  5             emb_dim = 70: IN > 1664, LgcpShape::nsk false, recompute by the library's own choice
  w1670-37  37   2  32 + 5
  cos       20   3  20            eps_schedule = "cos_sq", init_eps = 1e-3
  lin       20   3  20            eps_schedule = "linear"
  rc-n21    21   1  21            recompute: the side-stream hand-over at K = 1, where only one recompute runs ahead
  rc-n33    33   3  32 + 1        recompute: the buffer-set parity over three bridges
  rc-n65    65   2  32 + 32 + 1   recompute: three passes sharing the two event pairs
  var-*                           MCD_CAIS_var_sn (compute_log_var_grad), clipping on: n = 17 (merged, leaving at
                                  `if (!bptt) continue` before the third product), 21, 33, 52, and 21 at emb_dim = 12
  ulasn-*                         MCD_ULA_sn, K = 2, n = 17, 33, 52: the network's time index e - 1 lands in row 0 of S twice
  ula-*                           MCD_ULA (no network), K = 2, n = 6, 20, 33
  uha-*                           MCD_CAIS_UHA_sn (width 3220, 2 kNskChunks chunks, seven products per bridge): n = 16, 17, 20,
                                  21, 33 at K = 2 and n = 52 at K = 1: the no-split-K forward, the sweep on kept activations

The 2nd-order mode's other launch sequence (`uha_route`): the split-K forward (lgcp_uha_forward below its early return:
lgcp_uha_init_kernel unpacked, lgcp_gemm_kernel<EPI_NONE> on the 2 D-pitch state, lgcp_net_splitk with slabs and arrival counters,
lgcp_uha_mid_kernel<4> / lgcp_uha_close_kernel<4> summing kSplit slabs) and the recompute sweep (the `!kept` branch of
lgcp_uha_grad: kr_at, lgcp_uha_gather_kernel, two lgcp_net_splitk per bridge into the two LgcpFwdSets, the EPI_ACTB products
writing U1 / U2, the kSplit sums of the lgcp_uha_adj_* kernels), pinned by form 3 or taken by the library itself at IN > 3328.

  id            n    K  form  over         what it reaches
  uha-rc-n1     1    2  3                  one row: dim3(cb, kSplit) grids with M = 1, both buffer sets
  uha-rc-n20    20   2  3                  the configuration's pass (the merged instance on the kept path; no such split here)
  uha-rc-n21    21   1  3                  K = 1: kr_at(K) and kr_at(0) with one bridge between; the first boundary is the last
  uha-rc-n33    33   3  3                  32 + 1: counters and forward buffers reused by a second pass, the `base > 0` clear, three
                                           bridges through the two buffer sets
  uha-rc-n65    65   2  3                  three passes
  uha-w3332-5   5    2  0     emb_dim=132  IN = 3332 > 32 kNskChunks: the split-K form by the library's own choice; cbIN = 53
                                           with a 4-column last block
  uha-w3332-37  37   2  0     emb_dim=132  the same over 32 + 5
  uha-w3328-20  20   2  0     emb_dim=128  the last width the no-split-K form takes (exactly 2 x 104 chunks), merged pass
  uha-w3212-37  37   2  0     emb_dim=12   kept path at tIN = 201 with a ragged last tile, both GEMM families (32 + 5)
  uha-w3204-20  20   2  0     emb_dim=4    kept path, merged pass, IN % 16 = 4

The route the library takes in production when the kept tables pass 2^28 floats (`uha_keep_floats`; at width 3220 from
K n = 15 183 on whatever K is, e.g. K = 128 with n >= 119: `UHA_KEEP_OFF_KN`) is the no-split-K forward followed by the
recompute sweep.  No case can afford it as one call (2 K n > 27 000 evaluations of a 3220-wide network, and float64 autograd
through them); its two halves are pinned separately, the forward by the uha-* cases at form 0 and the sweep by the uha-rc-*
and uha-w3332-* cases.

Blocks (`blocks`): every leaf cut where different code writes it, each block scaled by its own maximum — see `blocks`.
Bars (`bars`): DESIGN.md section 2, "Gradients at d = 1600".  The reference of the bars is the restatement's own float32 against
float64 gap on the case's seeds (`float32_gap`, stored in tests/golden/lgcp_grad_gaps.json for the blocks above LISTED and
re-measured by tests/test_oracle_lgcp_grad.py); no bar comes from what a kernel returned.
"""
import functools
import json
import os

import numpy as np
import torch

from cmcd_amd import synthetic
from oracle import cmcd_oracle_torch as ot

from helpers import lgcp_counts_fixture

CAIS, VAR, ULASN, ULA, UHA = "MCD_CAIS_sn", "MCD_CAIS_var_sn", "MCD_ULA_sn", "MCD_ULA", "MCD_CAIS_UHA_sn"
CLIP = dict(grad_clipping=True)
LGCP_PASS = 32                  # kMP of cmcd_lgcp.hip
D = 1600

CASES = [
    # ---- overdamped, reparameterised, the library's choice of form
    ("n1", CAIS, 1, 2, 0, {}),
    ("n16", CAIS, 16, 2, 0, {}),
    ("n17", CAIS, 17, 2, 0, CLIP),
    ("n20", CAIS, 20, 2, 0, CLIP),
    ("n21", CAIS, 21, 1, 0, {}),
    ("n32", CAIS, 32, 2, 0, {}),
    ("n33", CAIS, 33, 3, 0, {}),
    ("n52", CAIS, 52, 2, 0, CLIP),
    ("n65", CAIS, 65, 2, 0, CLIP),
    ("n129", CAIS, 129, 1, 0, {}),
    ("w1612-21", CAIS, 21, 2, 0, dict(emb_dim=12)),
    ("w1612-37", CAIS, 37, 2, 0, dict(emb_dim=12)),
    ("w1604", CAIS, 20, 2, 0, dict(emb_dim=4)),
    ("w1670-5", CAIS, 5, 2, 0, dict(emb_dim=70)),
    ("w1670-37", CAIS, 37, 2, 0, dict(emb_dim=70)),
    ("cos", CAIS, 20, 3, 0, dict(eps_schedule="cos_sq", init_eps=1e-3)),
    ("lin", CAIS, 20, 3, 0, dict(eps_schedule="linear")),
    # ---- the recompute form
    ("rc-n21", CAIS, 21, 1, 3, {}),
    ("rc-n33", CAIS, 33, 3, 3, {}),
    ("rc-n65", CAIS, 65, 2, 3, {}),
    # ---- VarGrad, clipping on
    ("var-n17", VAR, 17, 2, 0, CLIP),
    ("var-n21", VAR, 21, 2, 0, CLIP),
    ("var-n33", VAR, 33, 2, 0, CLIP),
    ("var-n52", VAR, 52, 2, 0, CLIP),
    ("var-w1612", VAR, 21, 2, 0, dict(grad_clipping=True, emb_dim=12)),
    # ---- the overdamped baselines
    ("ulasn-n17", ULASN, 17, 2, 0, {}),
    ("ulasn-n33", ULASN, 33, 2, 0, {}),
    ("ulasn-n52", ULASN, 52, 2, 0, {}),
    ("ula-n6", ULA, 6, 2, 0, {}),
    ("ula-n20", ULA, 20, 2, 0, {}),
    ("ula-n33", ULA, 33, 2, 0, {}),
    # ---- 2nd order
    ("uha-n16", UHA, 16, 2, 0, {}),
    ("uha-n17", UHA, 17, 2, 0, {}),
    ("uha-n20", UHA, 20, 2, 0, {}),
    ("uha-n21", UHA, 21, 2, 0, {}),
    ("uha-n33", UHA, 33, 2, 0, {}),
    ("uha-n52", UHA, 52, 1, 0, {}),
    # ---- 2nd order: the split-K forward and the recompute sweep, pinned (form 3) ...
    ("uha-rc-n1", UHA, 1, 2, 3, {}),
    ("uha-rc-n20", UHA, 20, 2, 3, {}),
    ("uha-rc-n21", UHA, 21, 1, 3, {}),
    ("uha-rc-n33", UHA, 33, 3, 3, {}),
    ("uha-rc-n65", UHA, 65, 2, 3, {}),
    # ---- ... by the library's own choice (IN = 3332), at the last no-split-K width (3328), and the kept path at ragged widths
    ("uha-w3332-5", UHA, 5, 2, 0, dict(emb_dim=132)),
    ("uha-w3332-37", UHA, 37, 2, 0, dict(emb_dim=132)),
    ("uha-w3328-20", UHA, 20, 2, 0, dict(emb_dim=128)),
    ("uha-w3212-37", UHA, 37, 2, 0, dict(emb_dim=12)),
    ("uha-w3204-20", UHA, 20, 2, 0, dict(emb_dim=4)),
]
IDS = [c[0] for c in CASES]
PARAM_SETS = ("sparse", "dense")

# what a case says about its passes (tests/test_oracle_lgcp_grad.py re-derives it from n)
PASSES = {
    "n1": [1], "n16": [16], "n17": [17], "n20": [20], "n21": [21], "n32": [32], "n33": [32, 1], "n52": [32, 20],
    "n65": [32, 32, 1], "n129": [32, 32, 32, 32, 1], "w1612-21": [21], "w1612-37": [32, 5], "w1604": [20], "w1670-5": [5],
    "w1670-37": [32, 5], "cos": [20], "lin": [20], "rc-n21": [21], "rc-n33": [32, 1], "rc-n65": [32, 32, 1],
    "var-n17": [17], "var-n21": [21], "var-n33": [32, 1], "var-n52": [32, 20], "var-w1612": [21],
    "ulasn-n17": [17], "ulasn-n33": [32, 1], "ulasn-n52": [32, 20], "ula-n6": [6], "ula-n20": [20], "ula-n33": [32, 1],
    "uha-n16": [16], "uha-n17": [17], "uha-n20": [20], "uha-n21": [21], "uha-n33": [32, 1], "uha-n52": [32, 20],
    "uha-rc-n1": [1], "uha-rc-n20": [20], "uha-rc-n21": [21], "uha-rc-n33": [32, 1], "uha-rc-n65": [32, 32, 1],
    "uha-w3332-5": [5], "uha-w3332-37": [32, 5], "uha-w3328-20": [20], "uha-w3212-37": [32, 5], "uha-w3204-20": [20],
}
UHA_IDS = [c[0] for c in CASES if c[1] == UHA]


def case_by_id(cid):
    return next(c for c in CASES if c[0] == cid)


def passes_of(n):
    """The pass sizes of an n-particle call: whole passes of kMP, then the rest."""
    return [LGCP_PASS] * (n // LGCP_PASS) + ([n % LGCP_PASS] if n % LGCP_PASS else [])


def gemm_of(m):
    """Which product kernel a pass of m rows takes on kept activations."""
    return "nsk" if m <= 16 else "merged" if m <= 20 else "split-k"


# ---- the 2nd-order mode's launch rules, restated from cmcd_lgcp.hip (lgcp_shape's nsk rule, lgcp_uha_grad_ws)
NSK_CHUNKS = 104                # kNskChunks: 16-deep chunks of a packed operand
KEEP_FLOATS = 1 << 28           # cap of the tables the forward keeps for the sweep


def uha_nsk_ok(dim, emb_dim, form):
    """lgcp_shape's nsk rule at width 2 d: the no-split-K forward serves d <= 1664 in whole 16-column tiles and widths up to two rounds of chunks."""
    return form != 3 and dim % 16 == 0 and dim <= 16 * NSK_CHUNKS and 2 * dim + emb_dim <= 32 * NSK_CHUNKS


def uha_keep_floats(dim, emb_dim, K, n):
    """Floats of the kept tables (lgcp_uha_grad_ws): pre1, pre2 [2 K n][IN], sn [2 K n][D], kr [(K + 1) n][D]; u1 / u2 go to the
    tables the sweep has anyway."""
    IN, R = 2 * dim + emb_dim, 2 * K * n
    return R * (2 * IN + dim) + (K + 1) * n * dim


def uha_route(dim, emb_dim, K, n, form):
    """-> (forward, sweep) of a 2nd-order gradient call: "nsk" / "split-k", "kept" / "recompute"."""
    nsk = uha_nsk_ok(dim, emb_dim, form)
    kept = nsk and uha_keep_floats(dim, emb_dim, K, n) <= KEEP_FLOATS
    return "nsk" if nsk else "split-k", "kept" if kept else "recompute"


def route_of(case):
    _, mode, n, K, form, over = case
    assert mode == UHA
    return uha_route(D, over.get("emb_dim", 20), K, n, form)


# what each 2nd-order case says about its route (tests/test_oracle_lgcp_grad.py re-derives it)
UHA_ROUTES = {
    "uha-n16": ("nsk", "kept"), "uha-n17": ("nsk", "kept"), "uha-n20": ("nsk", "kept"), "uha-n21": ("nsk", "kept"),
    "uha-n33": ("nsk", "kept"), "uha-n52": ("nsk", "kept"),
    "uha-rc-n1": ("split-k", "recompute"), "uha-rc-n20": ("split-k", "recompute"), "uha-rc-n21": ("split-k", "recompute"),
    "uha-rc-n33": ("split-k", "recompute"), "uha-rc-n65": ("split-k", "recompute"),
    "uha-w3332-5": ("split-k", "recompute"), "uha-w3332-37": ("split-k", "recompute"),
    "uha-w3328-20": ("nsk", "kept"), "uha-w3212-37": ("nsk", "kept"), "uha-w3204-20": ("nsk", "kept"),
}
# Width 3220: the tables are K n (2 (2 IN + D) + D) + n D = 17 680 K n + 1600 n floats, so where `keep` turns off depends on K n
# and, weakly, on n.  The first K n at which it is off: 13 924 at K = 1, 15 183 as n -> 1; at the configuration's K = 128 the
# first n is 119 (K n = 15 232).  (Asserted on the CPU from uha_keep_floats.)
UHA_KEEP_OFF_KN = dict(k1=13924, any=15183)
UHA_KEEP_OFF_N_AT_K128 = 119


def seeds_of(case):
    return synthetic.parity_seeds(case[2])


def build(case, param_set, device="cuda"):
    """synthetic.build of the case on the parameter set ("sparse" / "dense"); -> its dict."""
    _, mode, n, K, _, over = case
    kw = dict(init_eps=0.02, init_gamma=5.0) if mode == UHA else dict(init_eps=2e-3)
    kw.update(over)
    return synthetic.build("lgcp_n20_k128", device=device, lgcp_counts=lgcp_counts_fixture(), nbridges=K, N=n, boundmode=mode,
                           dense=param_set == "dense", **kw)


def call(b, seeds, **kw):
    """The gradient call of the case's mode on device seeds -> (grad_flat, (losses, z))."""
    from cmcd_amd import mcdboundingmachine as mcdbm
    fn = mcdbm.compute_log_var_grad if b["params_fixed"][2] == VAR else mcdbm.compute_bound_grad
    return fn(seeds, b["params_flat"], b["unflatten"], b["params_fixed"], b["target"], eps_schedule=b["eps_schedule"],
              grad_clipping=b["grad_clipping"], **kw)


def forward(b, seeds):
    """The forward-only call on the same inputs -> (losses, z, stats)."""
    from cmcd_amd import mcdboundingmachine as mcdbm
    return mcdbm.bound_forward(seeds, b["params_flat"], b["unflatten"], b["params_fixed"], b["target"],
                               eps_schedule=b["eps_schedule"], grad_clipping=b["grad_clipping"])


# ------------------------------------------------------------------------------------------ the restatement
def oracle_params_of(b):
    """The restatement's parameter dict (float64 NumPy); MCD_ULA keeps no network."""
    un = b["unflatten"]
    if b["params_fixed"][2] != ULA:
        return synthetic.oracle_params(un, b["params_flat"])
    train, notrain = un(b["params_flat"].detach().cpu())
    allp = {**train, **notrain}
    f = lambda t: np.asarray(t.numpy(), np.float64)
    return {"vd": {k: f(v) for k, v in allp["vd"].items()}, "eps": f(allp["eps"]), "mgridref_y": f(allp["mgridref_y"]),
            "gridref_x": f(allp["gridref_x"]), "target_x": f(allp["target_x"])}


_LEAF_OF = {("eps",): ("eps",), ("gamma",): ("gamma",), ("mgridref_y",): ("mgridref_y",), ("vd", "mean"): ("vd", "mean"),
            ("vd", "logdiag"): ("vd", "logdiag"), ("sn", "emb"): ("sn", "emb"), ("sn", "factor_sn"): ("sn", "factor_sn"),
            ("sn", "nn", 0, 0): ("sn", "W1"), ("sn", "nn", 0, 1): ("sn", "b1"), ("sn", "nn", 1, 0): ("sn", "W2"),
            ("sn", "nn", 1, 1): ("sn", "b2"), ("sn", "nn", 2, 0): ("sn", "W3"), ("sn", "nn", 2, 1): ("sn", "b3")}


def flat_of(un, g, numel):
    """The restatement's gradient dict in params_flat order (float64); leaves it does not hold (eta, the two fixed grids, gamma
    outside the 2nd-order mode) are zero, as mcdboundingmachine returns them."""
    flat = np.zeros(numel, np.float64)
    for path, (off, shape) in un.layout.items():
        src = _LEAF_OF.get(tuple(path[1:])) if path[0] == 0 else None
        d = g
        for k in src or ():
            d = d.get(k) if isinstance(d, dict) else None
        if src is not None and d is not None:
            flat[off:off + max(1, int(np.prod(shape)))] = np.asarray(d, np.float64).reshape(-1)
    return flat


def run_restatement(case, param_set, dtype=torch.float64, seeds=None, logp=None):
    """ot.bound_and_grad of the case -> (value, losses, z, flat gradient in params_flat order), float64 NumPy."""
    b = build(case, param_set, device="cpu")
    seeds = seeds_of(case) if seeds is None else seeds
    logp = ot.make_logp_lgcp(lgcp_counts_fixture()) if logp is None else logp
    # float32: on at most GAP_THREADS threads.  The summation order of the float32 products follows the thread count, and a gap
    # that is one scalar's error (eps under VarGrad) moves with it; the stored gaps were measured at GAP_THREADS.
    threads = torch.get_num_threads()
    if dtype == torch.float32 and threads > GAP_THREADS:
        torch.set_num_threads(GAP_THREADS)
    try:
        val, l, z, g = _bound_and_grad(b, seeds, logp, dtype)
    finally:
        torch.set_num_threads(threads)
    return val, np.asarray(l, np.float64), np.asarray(z, np.float64), flat_of(b["unflatten"], g, b["params_flat"].numel())


GAP_THREADS = 8


def _bound_and_grad(b, seeds, logp, dtype):
    dim, K, mode, spec = b["params_fixed"]
    return ot.bound_and_grad(seeds, oracle_params_of(b), dim, K, mode, "geffner" if spec is None else spec.arch, logp,
                             b["cfg"]["eps_schedule"], b["cfg"]["grad_clipping"], dtype=dtype)


@functools.lru_cache(maxsize=2)          # a 2nd-order gradient is 200 MB of float64: the tests of a case run back to back
def _reference(cid, param_set):
    return run_restatement(case_by_id(cid), param_set)


def reference(case, param_set):
    """The float64 restatement on the case's seeds, computed once per (case, parameter set) and shared (read-only)."""
    return _reference(case[0], param_set)


# ------------------------------------------------------------------------------------------ blocks
def blocks(un, flat):
    """-> [(name, array view, covers)]: the leaves of a flat gradient cut where different code writes them.
      W1                 state rows [:D] (lgcp_tn_gemm_kernel, X^T dA1) against the emb_dim embedding rows
                         (launch_geffner_tails, out of the S table), each split at the last emb_dim columns (they sit behind the
                         last full 16- and 128-column tile); in the 2nd-order mode the state rows are `W1.z` [:D] and `W1.rho`
                         [D:2D]: the two halves of XIN's rows are written by different code (lgcp_uha_xin_kernel /
                         lgcp_uha_gather_kernel copy z once and rho, rho' apart), and the rho rows are the smaller ones;
      W2, b1, b2         the same column split;
      W3, b3             the last 64 columns (the last column block of cbD) against the rest;
      emb                per row (one per time index);
      mgridref_y, eps    per entry;
      factor_sn, gamma, eta, gridref_x, target_x   whole;
      vd.mean, vd.logdiag   per 64-column block (lgcp_colsum_kernel accumulates them over passes), and whole.
    `covers`: the block belongs to the cut that tiles its leaf exactly once (False for the two whole-leaf repeats of vd)."""
    out = []
    for path, (off, shape) in un.layout.items():
        a = flat[off:off + max(1, int(np.prod(shape)))].reshape(shape)
        key = tuple(path[1:])
        name = {("sn", "nn", 0, 0): "W1", ("sn", "nn", 0, 1): "b1", ("sn", "nn", 1, 0): "W2", ("sn", "nn", 1, 1): "b2",
                ("sn", "nn", 2, 0): "W3", ("sn", "nn", 2, 1): "b3"}.get(key, ".".join(map(str, key[-2:] if key[0] == "vd" else key[-1:])))
        if name in ("W1", "W2", "b1", "b2"):
            IN = shape[-1]
            emb = un.shape("sn", "emb")[1]
            d = un.shape("vd", "mean")[0]
            if name != "W1":
                rows = [("", slice(None))]
            elif IN - emb == d:
                rows = [(".state", slice(0, d)), (".emb", slice(d, IN))]
            else:
                rows = [(".z", slice(0, d)), (".rho", slice(d, 2 * d)), (".emb", slice(2 * d, IN))]
            for rn, rs in rows:
                sub = a[rs] if a.ndim == 2 else a
                out.append((name + rn + ".cols", sub[..., :IN - emb], True))
                out.append((name + rn + ".lastcols", sub[..., IN - emb:], True))
        elif name in ("W3", "b3"):
            out.append((name + ".cols", a[..., :shape[-1] - 64], True))
            out.append((name + ".last64", a[..., shape[-1] - 64:], True))
        elif name == "emb":
            out += [("emb[%d]" % i, a[i], True) for i in range(shape[0])]
        elif name in ("mgridref_y", "eps") and a.ndim == 1:
            out += [("%s[%d]" % (name, i), a[i:i + 1], True) for i in range(shape[0])]
        elif key[0] == "vd":
            out += [("%s[%d:%d]" % (name, c, min(c + 64, shape[0])), a[c:c + 64], True) for c in range(0, shape[0], 64)]
            out.append((name, a, False))
        else:
            out.append((name, a.reshape(-1), True))
    return out


def block_errors(un, flat, flat_ref):
    """-> {block: (max |a - r|, max |r|)}."""
    return {name: (float(np.abs(a - r).max()), float(np.abs(r).max()))
            for (name, a, _), (_, r, _) in zip(blocks(un, flat), blocks(un, flat_ref))}


# ------------------------------------------------------------------------------------------ the float32 gap and the bars
BAR = 2e-3              # the suite's standard gradient bar (tests/test_gpu_grad.py:_compare)
QUARTER = 0.25          # ... which holds while the restatement's own float32 gap stays within this share of it
FACTOR = 4.0            # otherwise the bar is this multiple of the gap
LISTED = 1e-4           # the golden file lists the blocks whose gap is above this; every other block is asserted below 1.5 x it
LOST = 5e-2             # a float32 gap beyond this share of a block's scale: the gradient is no test of that block
MAX_LOST = 0.1          # at most this share of a case's blocks may be lost
TINY = 1e-12            # blocks whose reference maximum is below this are listed by name (golden "tiny")
SHARD_TOL = 1e-4        # test_reparameterised_gradient_shards_add_up: shards against the single call, of the maximum
GAPS_PATH = os.path.join(os.path.dirname(__file__), "golden", "lgcp_grad_gaps.json")


def worst_particle(l, l_ref):
    return float((np.abs(l - l_ref) / np.maximum(1.0, np.abs(l_ref))).max())


def z_error(z, z_ref):
    """Worst element of z against the scale helpers.compare_losses uses: max(1, p99 |z_ref|)."""
    return float(np.abs(z - z_ref).max()) / max(1.0, float(np.quantile(np.abs(z_ref), 0.99)))


def float32_gap(case, param_set):
    """The restatement at float32 against float64 on the case's seeds -> dict(loss = worst-particle relative loss error,
    z = worst z element over compare_losses' scale, blocks = {block: gap relative to the block's own maximum} for blocks with a
    non-zero reference, tiny = [blocks whose reference maximum is below TINY but not zero], zero = [exactly zero ones])."""
    b = build(case, param_set, device="cpu")
    _, l64, z64, g64 = reference(case, param_set)
    _, l32, z32, g32 = run_restatement(case, param_set, dtype=torch.float32)
    assert np.isfinite(l64).all() and np.isfinite(l32).all(), (case[0], "a non-finite reference loss")
    errs = block_errors(b["unflatten"], g32, g64)
    return dict(loss=worst_particle(l32, l64), z=z_error(z32, z64),
                blocks={k: e / s for k, (e, s) in errs.items() if s > 0.0},
                tiny=sorted(k for k, (e, s) in errs.items() if 0.0 < s < TINY),
                zero=sorted(k for k, (e, s) in errs.items() if s == 0.0))


@functools.lru_cache(maxsize=None)
def stored_gaps():
    with open(GAPS_PATH) as f:
        return json.load(f)


def stored_gap(case, param_set):
    """The golden record of `float32_gap`: loss, z, blocks (those above LISTED only), tiny, zero."""
    return stored_gaps()[case[0]][param_set]


def bar_of(gap):
    """The bar of a block whose float32 gap is `gap` (relative to the block's own maximum): BAR while the gap is within a quarter
    of it, FACTOR x the gap beyond, None (lost: no test of the block) beyond LOST."""
    if gap > LOST:
        return None
    return BAR if gap <= QUARTER * BAR else FACTOR * gap


def bars(case, param_set):
    """-> (bar of a block by name, [lost blocks]) from the stored gaps; an unlisted block has a gap below 1.5 x LISTED."""
    listed = stored_gap(case, param_set)["blocks"]
    return (lambda name: bar_of(listed.get(name, LISTED))), sorted(k for k, g in listed.items() if g > LOST)


def uha_loss_bars():
    """-> (bar of the worst-particle loss error, bar of z_error) of every 2nd-order case: FACTOR x the largest float32 gap of
    that metric the golden file stores for any uha-* case.  helpers.compare_losses' 1e-3 of a loss of 1e3 .. 1e4 nats is several
    nats: a missing column's term would pass it.  tests/test_oracle_lgcp_grad.py holds both within a quarter of that bar."""
    gaps = [stored_gaps()[cid][ps] for cid in UHA_IDS for ps in PARAM_SETS]
    return FACTOR * max(g["loss"] for g in gaps), FACTOR * max(g["z"] for g in gaps)


def compare_blocks(case, param_set, un, flat, flat_ref, tag="", bars_of=None, errors_of=None):
    """Every block of the HIP gradient against the reference under `bars`; a block whose reference is exactly zero must be
    exactly zero.  A bar is relative to the block's own maximum, whatever its size (no escape for small blocks: the tiny ones the
    golden file names get the same rule, i.e. an absolute bar of bar x their maximum, FACTOR x the float32 gap where that
    counts).  `bars_of` / `errors_of`: another table's `bars` and `block_errors` under the same rule (tests/grad_blocks.py: the
    small-d gradients and their cut).  -> ({block: error / scale}, [failures])."""
    bar, lost = (bars_of or bars)(case, param_set)
    rep, bad = {}, []
    for name, (e, s) in (errors_of or block_errors)(un, flat, flat_ref).items():
        if s == 0.0:
            if e != 0.0:
                bad.append("%s: expected exactly zero, got up to %.3e" % (name, e))
            continue
        rep[name] = e / s
        if name in lost:
            continue
        if not e <= bar(name) * s:
            bad.append("%s: %.3e of its maximum %.3e (bar %.1e)" % (name, e / s, s, bar(name)))
    return rep, ["%s %s" % (tag, m) for m in bad]
