"""The small-d training gradients (gmm, funnel, many_gmm) cut where different code writes them, the case table of every gradient
comparison of tests/test_gpu_grad.py, tests/test_gpu_uha.py and tests/test_gpu_ldvi.py, and the bars of the cut.

TEST INFRASTRUCTURE ONLY.  tests/test_oracle_grad_blocks.py asserts on the CPU, from the float64 restatement alone, that the cut
tiles every leaf once, that the stored float32 gaps (tests/golden/grad_block_gaps.json, `python tests/grad_blocks.py --write`) are
current (the committed file is `--write` followed by `--merge`, see the end of this file) and that the comparison sees what the
per-leaf one cannot; the GPU files run `compare_blocks` beside what they asserted
before.  The rule is tests/lgcp_grad_cases.py's, imported: a block is held to BAR of its OWN maximum while the restatement's
float32-against-float64 gap on the case's seeds stays within QUARTER of BAR, to FACTOR x that gap beyond, and is lost beyond LOST
(at most MAX_LOST of the blocks of a (case, parameter set)); a block whose reference is exactly zero must be exactly zero; no
escape for small blocks.  No bar comes from what a kernel returned.

Why per block: a leaf's maximum hides its smaller parts.  On the 132-wide net under VarGrad the 130 embedding rows of dW1 (98 % of
the leaf) lie below 2e-3 of the leaf's maximum, which sits in the two state rows: a tail that wrote zeros there passes the leaf bar
and costs the cosine 3e-8.

The cut (`blocks`), read against cmcd_grad.hip, cmcd_bptt.hip, the sweep of cmcd_uha.hip and cmcd_ldvi.hip.  H = the net's width,
D = dim; a 16-unit tile is one matrix-instruction tile of the kernels, the last tile of a 132- / 134-wide net holds 4 / 6 real units:

  geffner net
    W1.state / W1.z, W1.rho   the state rows [:D] (2nd-order and LDVI trees: z rows [:D], rho rows [D:2D]): the per-wave accZ1 regions
                     of the slabs (grad_kernel, bptt / uha / ldvi sweeps), summed by grad_reduce_body (`perwave`); per 16-column tile
    W1.emb           the embedding rows: the geffner tail (grad_geffner_tail_body: dW1[D + j][n] = sum_e emb[ie][j] S[e][n] out of
                     the bias-table sums S); per 16-column tile
    b1               the same tail (db1[n] = sum_e S[e][n]); per 16-unit tile
    W2               the slab's HP x HP region, row tiles dealt over the waves, summed over slabs by grad_reduce_body; 16 x 16 tiles
    b2               the per-wave regions; per 16-unit tile
    W3               the slab's HP x 16 region; per 16-row tile
    b3, factor_sn    the per-wave regions; whole
    emb              the geffner tail, one wave per (row, j): S2[e][D + j] + W1[D + j] . S[e]; row K - 1 collects the evaluations
                     K - 1 and K (MCD_ULA_sn: row 0 collects two); per row
  dds net
    timestep_phase, linear/w, linear/b, linear_1/w, linear_1/b   the dds tail (grad_dds_tail_body per evaluation, then
                     grad_dds_tail_sum_kernel's fixed-order sum over evaluations); phase whole, weights per 16-column tile, biases per
                     16-unit tile
    linear_2/w       state rows [:D] (2nd-order trees: z rows [:D] and rho rows [D:2D]; the per-wave accZ1 regions) against the
                     last 64 rows, the time embedding (the dds tail: tau(e) x S[e]); each per 16-column tile;  linear_2/b from the
                     same tail, per 16-unit tile
    linear_3/w       16 x 16 tiles;  linear_3/b per 16-unit tile;  linear_zero/w per 16-row tile;  linear_zero/b whole
  every tree
    eps              the schedule tail (grad_sched_tail_body: sum_i geps[i] d eps_i / d eps0); whole
    mgridref_y       the schedule tail, per entry: node q collects the upper ends of cell q and the lower ends of cell q + 1, so the
                     first and the last entry are one-sided
    gamma, eta       whole (gamma is a trained leaf in the 2nd-order and LDVI modes only; eta has no gradient anywhere)
    vd.mean, vd.logdiag   the per-wave regions (ula_vd_reduce_kernel without a network); per coordinate
    gridref_x, target_x   params_notrain: whole, exactly zero

Cases.  A case is `(id, config, n, overrides)` in the table of its family; the seeds are synthetic.parity_seeds(n) (the gated cases
bring their own), every case runs on both parameter sets (LDVI: the dense one alone, as tests/ldvi_cases.py builds it).  The tables
keep the order and the values the GPU files had, so that every test keeps its id; a case's id says family, target, what is special
and n.  New in this table, each at an edge of a block's writer that had no case:

  var-many-w132-n49   132-wide net, VarGrad, both gradient paths: four particle tiles with three tiles per workgroup, so the second
                      workgroup has one live wave; the 4-unit last neuron tile of W1.emb / W2 / b1 / b2 written from there
  sn-many-w132-n49    the same net and batch through the reparameterised sweep (cmcd_bptt.hip), all forward variants
  uha-many-w134-n17   the 134-wide 2nd-order net at a one-particle second tile: W1.z against W1.rho on 9 neuron tiles, 6 units last
  sn-funnel-dds-k1    dds on the funnel at K = 1: the time-embedding rows of linear_2/w out of a single table row pair (e = 0, 1)
  sn-gmm-k1           geffner, K = 1 at n = 33: emb has one row, fed by both evaluations; mgridref_y's two entries both one-sided

LDVI: every case of tests/ldvi_cases.py under the id "ldvi-<id>" but gmm-nw4 and gmm-nw8 (16 400 and 131 088 particles: their
float64 restatement is what the CPU suite can afford, a second cut of it is not; they keep the leaf comparison alone).
"""
import contextlib
import functools
import json
import os
import sys
from functools import partial

import numpy as np
import torch

if __name__ == "__main__":      # run as a script: the repository root is not on the path yet (under pytest conftest.py puts it there)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cmcd_amd import synthetic
from oracle import cmcd_oracle_torch as ot

import gated_cases as gc
import lgcp_grad_cases as lg
from lgcp_grad_cases import BAR, FACTOR, GAP_THREADS, LISTED, LOST, MAX_LOST, QUARTER, TINY, bar_of  # noqa: F401  (the rule, imported)

GAPS_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "grad_block_gaps.json")
PARAM_SETS = ("sparse", "dense")
VARGRAD, SN, ULASN, ULA, UHA = "MCD_CAIS_var_sn", "MCD_CAIS_sn", "MCD_ULA_sn", "MCD_ULA", "MCD_CAIS_UHA_sn"
_MANY, _MANYVAR, _GMM, _FUNNEL = "many_gmm_n2000_k256_dds", "many_gmm_var_n16000_k256", "gmm_n300_k8", "funnel_n300_k64"

# ---- VarGrad (tests/test_gpu_grad.py: CASES)
VAR_CASES = [
    ("var-many-dds-n96", _MANY, 96, dict(boundmode=VARGRAD, nbridges=8, init_sigma=15.0)),
    ("var-many-dds-lin-n50", _MANY, 50, dict(boundmode=VARGRAD, nbridges=5, init_sigma=15.0, eps_schedule="linear", init_eps=0.3)),
    ("var-gmm-clip-n128", _GMM, 128, dict(boundmode=VARGRAD, grad_clipping=True)),
    ("var-funnel-n70", _FUNNEL, 70, dict(boundmode=VARGRAD, nbridges=6)),
    ("var-funnel-e20-n40", _FUNNEL, 40, dict(boundmode=VARGRAD, nbridges=5, emb_dim=20)),        # the default emb_dim: width 30 -> 64
    ("var-funnel-dds-n40", _FUNNEL, 40, dict(boundmode=VARGRAD, nbridges=5, nn_arch="dds")),
    ("var-many-e20-n64", _MANYVAR, 64, dict(nbridges=6, emb_dim=20)),
    ("var-many-w132-n80", _MANYVAR, 80, dict(nbridges=5)),                # 132-wide net (config 4), 3-wave groups
    ("var-many-e40-n60", _MANYVAR, 60, dict(nbridges=6, emb_dim=40)),     # the reference README's example width (42 -> padded to 64)
    ("var-many-e70-n40", _MANYVAR, 40, dict(nbridges=4, emb_dim=70)),     # width 72 -> padded to 144
    ("var-gmm-e90-n40", _GMM, 40, dict(boundmode=VARGRAD, nbridges=4, emb_dim=90)),   # 9 tiles on gmm
    ("var-many-w132-n49", _MANYVAR, 49, dict(nbridges=5)),                # new: a second workgroup with one live wave
]

# ---- the reparameterised gradient (BPTT_CASES): no stop_gradient, back-propagation through all K steps
BPTT_CASES = [
    ("sn-many-dds-n96", _MANY, 96, dict(nbridges=8, init_sigma=15.0)),                       # clipping on, cos_sq
    ("sn-many-dds-lin-n50", _MANY, 50, dict(nbridges=5, init_sigma=15.0, eps_schedule="linear", init_eps=0.3, grad_clipping=False)),
    ("sn-many-dds-k24-n40", _MANY, 40, dict(nbridges=24, init_sigma=15.0, init_eps=0.2)),    # longer chain
    ("sn-gmm-n128", _GMM, 128, dict()),                                                      # geffner 22
    ("sn-gmm-dds-clip-n64", _GMM, 64, dict(nn_arch="dds", grad_clipping=True)),
    ("sn-funnel-n70", _FUNNEL, 70, dict(nbridges=6)),                                        # d = 10, geffner 58
    ("sn-funnel-e20-n40", _FUNNEL, 40, dict(nbridges=5, emb_dim=20)),                        # default emb_dim (width 30 -> 64)
    ("sn-funnel-dds-n40", _FUNNEL, 40, dict(nbridges=5, nn_arch="dds")),
    ("sn-many-e20-n64", _MANY, 64, dict(nbridges=6, nn_arch="geffner", emb_dim=20, init_sigma=15.0, init_eps=0.3)),
    ("sn-many-e40-n48", _MANY, 48, dict(nbridges=5, nn_arch="geffner", emb_dim=40, init_sigma=15.0, init_eps=0.3)),   # width 42 -> 64
    ("sn-gmm-e7-n50", _GMM, 50, dict(emb_dim=7)),                                                                    # width 9 -> 32
    ("sn-many-e100-n40", _MANY, 40, dict(nbridges=4, nn_arch="geffner", emb_dim=100, init_sigma=15.0, init_eps=0.3)),  # 102 -> 144
    ("sn-gmm-e130-n40", _GMM, 40, dict(nbridges=4, emb_dim=130)),                                                    # 9 tiles, gmm
    ("sn-many-w132-n49", _MANY, 49, dict(nbridges=4, nn_arch="geffner", emb_dim=130, init_sigma=15.0, init_eps=0.3)),  # new
    ("sn-funnel-dds-k1", _FUNNEL, 40, dict(nbridges=1, nn_arch="dds")),                                              # new
    ("sn-gmm-k1", _GMM, 33, dict(nbridges=1)),                                                                       # new
]

# ---- the overdamped baselines (ULA_CASES), once with the network in the backward kernel and once without a network
ULA_CASES = [
    ("many-n70", _MANY, 70, dict(nbridges=6, init_sigma=15.0, init_eps=0.2)),
    ("gmm-n96", _GMM, 96, dict()),
    ("funnel-n40", _FUNNEL, 40, dict(nbridges=5)),
]
ULASN_CASES = [("ulasn-" + c[0],) + c[1:] for c in ULA_CASES]
ULANET_CASES = [("ula-" + c[0],) + c[1:] for c in ULA_CASES]

# ---- the generic component loop of the target (test_gradient_with_a_17_component_mixture)
MIX17_CASE = ("sn-mix17-n80", _MANY, 80, dict(nbridges=6, n_mixes=17, init_sigma=15.0, init_eps=0.3))

# ---- test_gradient_edge_shapes: single particle, single bridge, ragged last tile, on gmm
EDGE_SHAPES = [(1, 1), (17, 2), (3, 1), (33, 3)]
EDGE_CASES = [("edge-%s-n%d-k%d" % ("sn" if mode == SN else "var", n, K), _GMM, n, dict(boundmode=mode, nbridges=K))
              for mode in (SN, VARGRAD) for n, K in EDGE_SHAPES]

# ---- 2nd-order CMCD (tests/test_gpu_uha.py: GRAD_CASES)
UHA_CASES = [
    ("uha-gmm-n128", _GMM, 128, {}),                                                               # geffner 24 (2 tiles)
    ("uha-gmm-dds-n64", _GMM, 64, dict(nn_arch="dds", init_gamma=3.0)),                             # dds on d = 2
    ("uha-many-dds-k8-n96", _MANY, 96, dict(nbridges=8, init_eps=0.2, init_gamma=2.0, init_sigma=15.0)),
    ("uha-many-dds-k24-n40", _MANY, 40, dict(nbridges=24, init_eps=0.1, init_gamma=3.0, init_sigma=15.0)),   # longer chain
    ("uha-funnel-n70", _FUNNEL, 70, dict(nbridges=6, init_eps=0.05, init_gamma=4.0)),               # d = 10, geffner 68 (5 tiles)
    ("uha-funnel-dds-n40", _FUNNEL, 40, dict(nbridges=5, nn_arch="dds", init_eps=0.05)),            # d = 10: two input tiles
    ("uha-funnel-e20-n40", _FUNNEL, 40, dict(nbridges=4, emb_dim=20, init_eps=0.05)),               # width 40 -> 64
    ("uha-many-w134-n80", _MANYVAR, 80, dict(nbridges=5, init_eps=0.1, init_gamma=3.0)),            # geffner 134 (9 tiles)
    ("uha-gmm-e40-n50", _GMM, 50, dict(emb_dim=40, nbridges=5)),                                    # width 44 -> 64
    ("uha-gmm-k3-n300", _GMM, 300, dict(nbridges=3)),                                               # 19 tiles: five workgroups, ragged
    ("uha-gmm-dds-k1-n20", _GMM, 20, dict(nbridges=1, nn_arch="dds")),                              # a single bridge
    ("uha-gmm-k40-n70", _GMM, 70, dict(nbridges=40, init_eps=0.05)),                                # 41 points: ten chunks of work items
    ("uha-funnel-k19-n50", _FUNNEL, 50, dict(nbridges=19, init_eps=0.03, init_gamma=4.0)),          # d = 10 in chunks
    ("uha-many-w134-n17", _MANYVAR, 17, dict(nbridges=5, init_eps=0.1, init_gamma=3.0)),            # new: a one-particle second tile
]

NEW_CASES = ("var-many-w132-n49", "sn-many-w132-n49", "sn-funnel-dds-k1", "sn-gmm-k1", "uha-many-w134-n17")
LDVI_LEAF_ONLY = ("gmm-nw4", "gmm-nw8")     # too large for a second float32 restatement in the CPU suite: the leaf comparison alone


def _ldvi_ids():
    import ldvi_cases
    return ["ldvi-" + c for c in ldvi_cases.CASES if c not in LDVI_LEAF_ONLY]


# family -> (table, mode; None: the case's own `boundmode`)
FAMILIES = {"var": (VAR_CASES, VARGRAD), "sn": (BPTT_CASES, SN), "ulasn": (ULASN_CASES, ULASN), "ula": (ULANET_CASES, ULA),
            "mix17": ([MIX17_CASE], SN), "edge": (EDGE_CASES, None), "uha": (UHA_CASES, UHA)}
GATED_IDS = ["gated-" + c[0] for c in gc.GATED_CASES]


@functools.lru_cache(maxsize=None)
def _index():
    out = {}
    for fam, (table, mode) in FAMILIES.items():
        for cid, config, n, over in table:
            assert cid not in out, cid
            out[cid] = dict(family=fam, config=config, n=n, over=over, mode=mode or over["boundmode"])
    for c in gc.GATED_CASES:
        out["gated-" + c[0]] = dict(family="gated", gated=c, n=len(c[3]), mode=c[4])
    for cid in _ldvi_ids():
        out[cid] = dict(family="ldvi", ldvi=cid[len("ldvi-"):])
    return out


def ids(*families):
    """The case ids of the named families (all of them without an argument), in table order."""
    return [cid for cid, c in _index().items() if not families or c["family"] in families]


def param_sets_of(cid):
    return ("dense",) if _index()[cid]["family"] == "ldvi" else PARAM_SETS


def records():
    """[(case id, parameter set)] of everything the golden file holds."""
    return [(cid, ps) for cid in ids() for ps in param_sets_of(cid)]


def cid_of(family, config, n, over):
    """The id of a table row by its values (the GPU files parametrise over the rows, which keeps their test ids)."""
    for cid, c, m, o in FAMILIES[family][0]:
        if (c, m, o) == (config, n, over):
            return cid
    raise KeyError((family, config, n, over))


def rows(family):
    """The table of a family without its ids: [(config, n, overrides)]."""
    return [c[1:] for c in FAMILIES[family][0]]


# ------------------------------------------------------------------------------------------ build and restatement
@contextlib.contextmanager
def _dense_default(dense):
    saved = synthetic.DENSE_DEFAULT
    synthetic.DENSE_DEFAULT = dense
    try:
        yield
    finally:
        synthetic.DENSE_DEFAULT = saved


def build(cid, param_set, device="cpu"):
    """The built case on the parameter set -> synthetic.build's dict."""
    c = _index()[cid]
    if c["family"] == "ldvi":
        import ldvi_cases
        assert param_set == "dense"
        return ldvi_cases.build(c["ldvi"], device=device)
    if c["family"] == "gated":
        with _dense_default(param_set == "dense"):
            return gc.build_case(c["gated"], device=device)
    return synthetic.build(c["config"], device=device, dense=param_set == "dense", **{**c["over"], "boundmode": c["mode"]})


def seeds_of(cid):
    c = _index()[cid]
    if c["family"] == "ldvi":
        import ldvi_cases
        return ldvi_cases.seeds_of(c["ldvi"])
    return np.asarray(c["gated"][3], np.int32) if c["family"] == "gated" else synthetic.parity_seeds(c["n"])


def _oracle_params(b):
    if b["params_fixed"][2] != ULA:
        return synthetic.oracle_params(b["unflatten"], b["params_flat"])
    return lg.oracle_params_of(b)          # MCD_ULA keeps no network


_GEFFNER = {("sn", "emb"): "emb", ("sn", "factor_sn"): "factor_sn", ("sn", "nn", 0, 0): "W1", ("sn", "nn", 0, 1): "b1",
            ("sn", "nn", 1, 0): "W2", ("sn", "nn", 1, 1): "b2", ("sn", "nn", 2, 0): "W3", ("sn", "nn", 2, 1): "b3"}
_DDS = {"linear": ("t_w1", "t_b1"), "linear_1": ("t_w2", "t_b2"), "linear_2": ("s_w1", "s_b1"), "linear_3": ("s_w2", "s_b2"),
        "linear_zero": ("s_w3", "s_b3")}


def _oracle_leaf(g, key):
    """The restatement's gradient of the leaf at layout key (path without its train / notrain index), or None."""
    if key[0] == "vd":
        return g["vd"][key[1]]
    if key[0] != "sn":
        return g.get(key[0])
    gs = g.get("sn")
    if gs is None:
        return None
    if key in _GEFFNER:
        return gs[_GEFFNER[key]]
    if key[1:] == ("drift_net", "timestep_phase"):
        return gs["timestep_phase"]
    return gs[_DDS[key[1].split("/")[-1]][0 if key[2] == "w" else 1]]


def flat_of(un, g, numel):
    """The restatement's gradient dict in params_flat order (float64 NumPy); a leaf it does not hold (eta, the two fixed grids)
    is zero, as the library returns it."""
    flat = np.zeros(numel, np.float64)
    for path, (off, shape) in un.layout.items():
        leaf = _oracle_leaf(g, tuple(path[1:])) if path[0] == 0 else None
        if leaf is not None:
            flat[off:off + max(1, int(np.prod(shape)))] = np.asarray(leaf, np.float64).reshape(-1)
    return flat


def _target_of(cid, b):
    n_mixes = _index()[cid].get("over", {}).get("n_mixes")
    return partial(ot.logp_many_gmm, n_mixes=n_mixes) if n_mixes else b["cfg"]["model"]


@contextlib.contextmanager
def _threads(dtype):
    """float32 on at most GAP_THREADS threads (the summation order of the float32 products follows the thread count)."""
    threads = torch.get_num_threads()
    if dtype == torch.float32 and threads > GAP_THREADS:
        torch.set_num_threads(GAP_THREADS)
    try:
        yield
    finally:
        torch.set_num_threads(threads)


def run_restatement(cid, param_set, dtype=torch.float64, params_edit=None):
    """-> (value, losses, z, flat gradient in params_flat order, the restatement's gradient dict), float64 NumPy.
    `params_edit(p)`: edits the restatement's parameter dict before the run (the planted slips of the CPU test)."""
    c = _index()[cid]
    b = build(cid, param_set)
    un, numel = b["unflatten"], b["params_flat"].numel()
    with _threads(dtype):
        if c["family"] == "ldvi":
            import ldvi_cases
            import ldvi_restatement as lr
            assert params_edit is None
            p, (dim, K, mode, _), model = ldvi_cases.params_of(c["ldvi"])
            if dtype == torch.float64:
                l, z, flat = ldvi_cases.reference(c["ldvi"])
            else:
                l, z, g = lr.bound_and_grad(seeds_of(cid), p, dim, K, model, use_sn=mode == "MCD_U_a-lp-sn", dtype=dtype)
                flat = lr.flat_grad(un, numel, g)
            return float(np.mean(l)), np.asarray(l, np.float64), np.asarray(z, np.float64), np.asarray(flat, np.float64), None
        dim, K, mode, spec = b["params_fixed"]
        p = _oracle_params(b)
        if params_edit is not None:
            params_edit(p)
        arch = "dds" if spec is None else spec.arch
        val, l, z, g = ot.bound_and_grad(seeds_of(cid), p, dim, K, mode, arch, _target_of(cid, b),
                                         None if mode == ULA else b["cfg"]["eps_schedule"],
                                         False if mode == ULA else b["cfg"]["grad_clipping"], dtype=dtype)
    flat = flat_of(un, g, numel) if params_edit is None else None      # an edited tree need not have the layout's shapes
    return val, np.asarray(l, np.float64), np.asarray(z, np.float64), flat, g


@functools.lru_cache(maxsize=None)
def reference(cid, param_set):
    """The float64 restatement on the case's seeds, once per (case, parameter set) and shared (read-only)
    -> (value, losses, z, flat gradient)."""
    out = run_restatement(cid, param_set)[:4]
    for a in out[1:]:
        a.setflags(write=False)
    return out


def reference_torch(cid, param_set):
    """`reference` as tests/test_gpu_grad.py:oracle_grad_flat returned it -> (value, losses, float64 torch flat gradient)."""
    val, l, _, flat = reference(cid, param_set)
    return val, l, torch.from_numpy(flat.copy())


# ------------------------------------------------------------------------------------------ the cut
def _tiles(n):
    return [(c, min(c + 16, n)) for c in range(0, n, 16)]


def blocks(un, flat):
    """-> [(name, array view, covers)]: the leaves of a flat gradient cut where different code writes them (the module docstring
    says who writes which).  `covers`: the block belongs to the cut that tiles its leaf exactly once — every block does here."""
    out = []
    D = un.shape("vd", "mean")[0]
    for path, (off, shape) in un.layout.items():
        a = flat[off:off + max(1, int(np.prod(shape)))].reshape(shape)
        key = tuple(path[1:])
        if path[0] == 1 or key[0] in ("eps", "gamma", "eta"):
            out.append((str(key[-1]), a.reshape(-1), True))
        elif key[0] == "mgridref_y":
            out += [("mgridref_y[%d]" % i, a[i:i + 1], True) for i in range(shape[0])]
        elif key[0] == "vd":
            out += [("vd.%s[%d]" % (key[1], i), a[i:i + 1], True) for i in range(shape[0])]
        elif key in _GEFFNER:
            name = _GEFFNER[key]
            if name == "W1":
                IN, E = shape[0], un.shape("sn", "emb")[1]
                groups = [("state", 0, D)] if IN - E == D else [("z", 0, D), ("rho", D, 2 * D)]
                assert groups[-1][2] == IN - E, (IN, E, D)
                for gname, r0, r1 in groups + [("emb", IN - E, IN)]:
                    out += [("W1.%s[:,%d:%d]" % (gname, c0, c1), a[r0:r1, c0:c1], True) for c0, c1 in _tiles(shape[1])]
            elif name == "W2":
                out += [("W2[%d:%d,%d:%d]" % (r0, r1, c0, c1), a[r0:r1, c0:c1], True)
                        for r0, r1 in _tiles(shape[0]) for c0, c1 in _tiles(shape[1])]
            elif name == "W3":
                out += [("W3[%d:%d]" % (r0, r1), a[r0:r1], True) for r0, r1 in _tiles(shape[0])]
            elif name in ("b1", "b2"):
                out += [("%s[%d:%d]" % (name, c0, c1), a[c0:c1], True) for c0, c1 in _tiles(shape[0])]
            elif name == "emb":
                out += [("emb[%d]" % i, a[i], True) for i in range(shape[0])]
            else:                                       # b3, factor_sn
                out.append((name, a.reshape(-1), True))
        elif key[1:] == ("drift_net", "timestep_phase"):
            out.append(("timestep_phase", a.reshape(-1), True))
        else:
            mod, kind = key[1].split("/")[-1], key[2]
            name = "%s.%s" % (mod, kind)
            if mod == "linear_zero":
                out += [(name, a.reshape(-1), True)] if kind == "b" else \
                       [("%s[%d:%d]" % (name, r0, r1), a[r0:r1], True) for r0, r1 in _tiles(shape[0])]
            elif kind == "b":
                out += [("%s[%d:%d]" % (name, c0, c1), a[c0:c1], True) for c0, c1 in _tiles(shape[0])]
            elif mod == "linear_3":
                out += [("%s[%d:%d,%d:%d]" % (name, r0, r1, c0, c1), a[r0:r1, c0:c1], True)
                        for r0, r1 in _tiles(shape[0]) for c0, c1 in _tiles(shape[1])]
            elif mod == "linear_2":
                T = shape[0] - 64                       # the state rows in front of the 64 time-embedding rows
                groups = [("state", 0, D)] if T == D else [("z", 0, D), ("rho", D, 2 * D)]
                assert groups[-1][2] == T, (shape, D)
                for gname, r0, r1 in groups + [("time", T, shape[0])]:
                    out += [("%s.%s[:,%d:%d]" % (name, gname, c0, c1), a[r0:r1, c0:c1], True) for c0, c1 in _tiles(shape[1])]
            else:                                       # linear, linear_1
                out += [("%s[:,%d:%d]" % (name, c0, c1), a[:, c0:c1], True) for c0, c1 in _tiles(shape[1])]
    return out


def _np64(x):
    return x.detach().double().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x, np.float64)


def block_errors(un, flat, flat_ref):
    """-> {block: (max |a - r|, max |r|)}."""
    flat, flat_ref = _np64(flat), _np64(flat_ref)
    return {name: (float(np.abs(a - r).max()), float(np.abs(r).max()))
            for (name, a, _), (_, r, _) in zip(blocks(un, flat), blocks(un, flat_ref))}


# ------------------------------------------------------------------------------------------ the float32 gap and the bars
def float32_gap(cid, param_set):
    """The restatement at float32 against float64 on the case's seeds -> dict(loss = worst finite particle's relative loss error,
    z = worst z element over compare_losses' scale, blocks = {block: gap relative to the block's own maximum} for the blocks with
    a non-zero reference, tiny = [blocks whose reference maximum is below TINY but not zero], zero = [exactly zero ones])."""
    un = build(cid, param_set)["unflatten"]
    _, l64, z64, g64 = reference(cid, param_set)
    _, l32, z32, g32, _ = run_restatement(cid, param_set, dtype=torch.float32)
    assert not np.isnan(l64).any() and np.array_equal(np.isinf(l32), np.isinf(l64)), (cid, "float32 floors other particles")
    f = np.isfinite(l64)
    errs = block_errors(un, g32, g64)
    return dict(loss=lg.worst_particle(l32[f], l64[f]) if f.any() else 0.0, z=lg.z_error(z32, z64),
                blocks={k: e / s for k, (e, s) in errs.items() if s > 0.0},
                tiny=sorted(k for k, (e, s) in errs.items() if 0.0 < s < TINY),
                zero=sorted(k for k, (e, s) in errs.items() if s == 0.0))


@functools.lru_cache(maxsize=None)
def stored_gaps():
    with open(GAPS_PATH) as f:
        return json.load(f)


def stored_gap(cid, param_set):
    """The golden record of `float32_gap`: loss, z, blocks (those above LISTED only), tiny, zero."""
    return stored_gaps()[cid][param_set]


def bars(cid, param_set):
    """-> (bar of a block by name, [lost blocks]) from the stored gaps; an unlisted block has a gap below 1.5 x LISTED."""
    listed = stored_gap(cid, param_set)["blocks"]
    return (lambda name: bar_of(listed.get(name, LISTED))), sorted(k for k, g in listed.items() if g > LOST)


def compare_blocks(cid, param_set, un, flat, flat_ref, tag=""):
    """lgcp_grad_cases.compare_blocks on this file's cut and bars -> ({block: error / scale}, [failures])."""
    return lg.compare_blocks(cid, param_set, un, _np64(flat), _np64(flat_ref), tag=tag or "%s/%s" % (cid, param_set),
                             bars_of=bars, errors_of=block_errors)


def report_blocks(cid, param_set, un, flat, flat_ref, tag=""):
    """`compare_blocks`, printing the worst block against its bar -> [failures]."""
    rep, bad = compare_blocks(cid, param_set, un, flat, flat_ref, tag)
    bar, lost = bars(cid, param_set)
    held = {k: v / bar(k) for k, v in rep.items() if k not in lost}
    if held:
        w = max(held, key=held.get)
        print("blocks %s/%s: %d, worst %s %.2e of its maximum (bar %.1e)" % (cid, param_set, len(rep), w, rep[w], bar(w)))
    return bad


def assert_blocks(cid, param_set, un, flat, flat_ref, tag=""):
    bad = report_blocks(cid, param_set, un, flat, flat_ref, tag)
    assert not bad, bad


def _round_up(x):
    """x rounded up to two significant digits (the record is an upper bound of what was measured)."""
    if x == 0.0:
        return 0.0
    q = 10.0 ** (np.floor(np.log10(x)) - 1)
    # (1 - 1e-12): a value that has two digits already stays; through the decimal string, so that the file holds 0.00014 and not
    # the binary product 0.00014000000000000001
    return float("%.1e" % (np.ceil(x / q * (1 - 1e-12)) * q))


def measure_all():
    """Every record of the table, measured here -> the golden file's dict (values rounded up to two digits, blocks above LISTED)."""
    torch.set_num_threads(min(torch.get_num_threads(), GAP_THREADS))
    out = {}
    for cid, ps in records():
        g = float32_gap(cid, ps)
        rec = dict(loss=_round_up(g["loss"]), z=_round_up(g["z"]), tiny=g["tiny"], zero=g["zero"],
                   blocks={k: _round_up(v) for k, v in sorted(g["blocks"].items()) if v > LISTED})
        out.setdefault(cid, {})[ps] = rec
        lost = [k for k, v in rec["blocks"].items() if v > LOST]
        print(cid, ps, "loss %.1e z %.1e listed %d of %d lost %s" % (rec["loss"], rec["z"], len(rec["blocks"]),
                                                                     len(g["blocks"]) + len(g["zero"]), lost), flush=True)
    return out


def larger_of(a, b):
    """Two measurements of the table -> per entry the larger one (a block one of them does not list is below LISTED there)."""
    out = {}
    assert set(a) == set(b)
    for cid in a:
        for ps in a[cid]:
            ra, rb = a[cid][ps], b[cid][ps]
            assert ra["tiny"] == rb["tiny"] and ra["zero"] == rb["zero"], (cid, ps)
            blocks = {k: max(ra["blocks"].get(k, 0.0), rb["blocks"].get(k, 0.0)) for k in sorted(set(ra["blocks"]) | set(rb["blocks"]))}
            out.setdefault(cid, {})[ps] = dict(loss=max(ra["loss"], rb["loss"]), z=max(ra["z"], rb["z"]), tiny=ra["tiny"],
                                               zero=ra["zero"], blocks=blocks)
    return out


def _dump(out, path):
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    # --write: measure here and store.  --measure PATH: measure here into another file.  --merge PATH: keep, per entry, the larger
    # of the stored value and PATH's.  The last digits of a float32 product follow the BLAS code path of the CPU, and the gap of a
    # single-entry block is one draw of that noise: THE COMMITTED FILE IS `--write` FOLLOWED BY `--merge` of a `--measure` taken
    # under another BLAS code path.  `--write` alone does not reproduce it and would lower some bars; after a re-write, merge again.
    if "--write" in sys.argv:
        _dump(measure_all(), GAPS_PATH)
    elif "--measure" in sys.argv:
        _dump(measure_all(), sys.argv[sys.argv.index("--measure") + 1])
    elif "--merge" in sys.argv:
        with open(sys.argv[sys.argv.index("--merge") + 1]) as f:
            other = json.load(f)
        _dump(larger_of(stored_gaps(), other), GAPS_PATH)
