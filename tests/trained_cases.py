"""Cases in the two regions of parameter space that training reaches and cmcd_amd.synthetic.build does not, shared by
tests/test_oracle_trained_params.py (which asserts on the CPU, from the oracles alone, that each case is what it says) and
tests/test_gpu_trained.py (the HIP path against the float64 oracle on the same seeds).

  (a) trained snapshots   tests/golden/trained_<id>.npz: the merged `params` dict (utils.params_to_numpy) at the end of the
                          project's own training run of the row, written by tools/make_trained_fixtures.py on the GPU.  They are
                          inputs only: every expected value comes from the oracle.
  (b) box corners         synthetic.build(dense=True) plus edits (those of gated_cases.build_case and GRID below), with eps / gamma
                          on a face of the box that opt.project and cmcd_adam_step clamp to (eps in [1e-7, 0.5], gamma >= 1e-3) and
                          mgridref_y entries at their floor 1e-3.

A case is `(id, config, overrides, seeds, mode)` as in tests/gated_cases.py.  A trained snapshot has config None (its flags are
TRAINED_ROWS[id]); mode "UHA" is the plain Hamiltonian AIS machine (cmcd_amd.hais; yardstick tests/hais_restatement.py), whose
corner case has config "hais:<target>".  `seeds` are the survivors of `synthetic.parity_seeds(n0)`, n0 = N0[id], under the guard
band of gated_cases (DELTA) around the floor, the clips and the dds clamp; at most one in eight may be dropped.
"""
import json
import math
import os

import numpy as np
import torch

import gated_cases as gc
from cmcd_amd import synthetic
from oracle import cmcd_oracle as orc
from oracle import cmcd_oracle_torch as ot

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODEL_CONFIG = {"gmm": "gmm_n300_k8", "funnel": "funnel_n300_k64", "many_gmm": "many_gmm_n2000_k256_dds"}

EPS_LO, EPS_HI, GAMMA_LO, GRID_FLOOR = 1e-7, 0.5, 1e-3, 1e-3      # the faces of opt.project's box

# ------------------------------------------------------------------------------------------ (a) trained snapshots
# Flags under the names of cmcd_amd.main.get_config.  `readme`: the line of the reference's README whose replicate command the
# row restates (nbridges, and for the 2 x 130-wide many_gmm row emb_dim, changed to the sizes a quick test can afford); rows
# without one take the gmm / funnel row's flags with the boundmode swapped and the base configuration's train_eps = True.
# `iters` is what tools/make_trained_fixtures.py ran: the README's 11 000 except on many_gmm, whose rows have no iteration
# flag (the base configuration's 150 000) and run 3 000 here.  many-var: the README's lr 5e-3 is for K = 256; at K = 16 the
# VarGrad run leaves the finite range after some 300 iterations (at lr 1e-3 after 1 300: the logged mean loss climbs from 28 to
# 2 000 first), so the row runs at lr 2e-4, where 3 000 iterations stay finite.
_GMM = dict(model="gmm", N=300, nbridges=8, nn_arch="geffner", emb_dim=20, init_eps=0.01, init_sigma=1.0, eps_schedule="",
            grad_clipping=False, lr=1e-3, iters=11000, train_vi=True, train_eps=False, train_betas=True, seed=1)
_FUNNEL = dict(model="funnel", N=300, nbridges=16, nn_arch="geffner", emb_dim=48, init_eps=0.1, init_sigma=1.0,
               eps_schedule="cos_sq", grad_clipping=False, lr=0.01, iters=11000, train_vi=True, train_eps=False,
               train_betas=True, seed=1)
TRAINED_ROWS = {
    "gmm-cais": dict(_GMM, boundmode="MCD_CAIS_sn", readme=73),
    "funnel-cais": dict(_FUNNEL, boundmode="MCD_CAIS_sn", readme=53),
    "many-dds": dict(model="many_gmm", boundmode="MCD_CAIS_sn", N=2000, nbridges=64, nn_arch="dds", emb_dim=20, init_eps=1.0,
                     init_sigma=60.0, eps_schedule="cos_sq", grad_clipping=True, lr=1e-3, iters=3000, train_vi=False,
                     train_eps=False, train_betas=True, seed=1, readme=26),
    "many-var": dict(model="many_gmm", boundmode="MCD_CAIS_var_sn", N=2000, nbridges=16, nn_arch="geffner", emb_dim=40,
                     init_eps=0.65, init_sigma=15.0, eps_schedule="", grad_clipping=True, lr=2e-4, iters=3000, train_vi=False,
                     train_eps=False, train_betas=True, seed=1, readme=30),
    "gmm-uha-sn": dict(_GMM, boundmode="MCD_CAIS_UHA_sn", train_eps=True, init_gamma=10.0, readme=None),
    "funnel-ula-sn": dict(_FUNNEL, boundmode="MCD_ULA_sn", train_eps=True, readme=None),
    "gmm-ula": dict(_GMM, boundmode="MCD_ULA", train_eps=True, readme=None),
    "funnel-uha": dict(_FUNNEL, boundmode="UHA", nbridges=8, lfsteps=2, init_eta=0.0, init_eps=0.01, lr=1e-3, train_eps=True,
                       readme=None),
}


def trainable_of(row):
    """cmcd_amd/main.py:204-229."""
    t = ("eta",) if row["boundmode"] == "UHA" else ("eta", "gamma")
    for flag, name in (("train_eps", "eps"), ("train_vi", "vd"), ("train_betas", "mgridref_y")):
        if row[flag]:
            t += (name,)
    return t


def fixture_path(cid):
    return os.path.join(GOLD, f"trained_{cid}.npz")


def save_fixture(path, row, params, made_by):
    """`params`: utils.params_to_numpy's nested dict.  Stored as float32 leaves `leaf_<i>` in tree order, their paths as a
    JSON list (`paths`), the run's flags (`flags`) and how the file was made (`made_by`)."""
    leaves = []

    def walk(node, prefix):
        if isinstance(node, dict):
            for k in node:
                walk(node[k], prefix + [k])
        elif isinstance(node, (list, tuple)):
            for i, v in enumerate(node):
                walk(v, prefix + [i])
        else:
            leaves.append((prefix, np.asarray(node, np.float32)))
    walk(params, [])
    np.savez_compressed(path, paths=json.dumps([p for p, _ in leaves]), flags=json.dumps(row), made_by=made_by,
                        **{"leaf_%03d" % i: a for i, (_, a) in enumerate(leaves)})


def load_fixture(cid):
    """-> (flags, {leaf path (tuple): float32 array})."""
    with np.load(fixture_path(cid)) as f:
        paths = json.loads(str(f["paths"]))
        return json.loads(str(f["flags"])), {tuple(p): f["leaf_%03d" % i] for i, p in enumerate(paths)}


def fill(flat, unflatten, leaves):
    """Copies `{leaf path: array}` into `flat` at the offsets of `unflatten`; every leaf must exist with the stored shape."""
    by_path = {path[1:]: v for path, v in unflatten.layout.items()}
    for path, arr in leaves.items():
        off, shape = by_path[path]
        assert tuple(arr.shape) == tuple(shape), (path, arr.shape, shape)
        flat[off:off + max(1, arr.size)] = torch.from_numpy(np.ascontiguousarray(arr, np.float32).reshape(-1))
    return flat


def initial_build(row):
    """The parameter tree the row's training started from (cmcd_amd/main.py:218-234 without mean-field pre-training), every leaf
    trainable so that a gradient comes back for each.  -> a built dict as synthetic.build returns (hais: see build_case)."""
    from cmcd_amd import mcdboundingmachine as mcdbm
    from cmcd_amd import variationaldist as vd
    if row["boundmode"] == "UHA":
        from cmcd_amd import hais
        dim = 10 if row["model"] == "funnel" else 2
        flat, un, fixed = hais.initialize(dim, nbridges=row["nbridges"], lfsteps=row["lfsteps"], eps=row["init_eps"],
                                          eta=row["init_eta"], vdparams=vd.initialize(dim, init_sigma=row["init_sigma"]),
                                          trainable=("eta", "eps", "vd", "mgridref_y", "md"), device="cpu")
        return dict(kind="hais", params_flat=flat, unflatten=un, params_fixed=fixed, target_name=row["model"])
    over = {k: row[k] for k in ("boundmode", "nbridges", "nn_arch", "emb_dim", "init_eps", "init_sigma", "eps_schedule",
                                "grad_clipping")}
    if "init_gamma" in row:
        over["init_gamma"] = row["init_gamma"]
    b = synthetic.build(MODEL_CONFIG[row["model"]], device="cpu", dense=False, **over)
    dim, K, mode, spec = b["params_fixed"]
    flat, un, fixed = mcdbm.initialize(dim=dim, nbridges=K, vdparams=vd.initialize(dim, init_sigma=row["init_sigma"]), eta=0.0,
                                       eps=row["init_eps"], gamma=row.get("init_gamma", 10.0),
                                       trainable=("eta", "gamma", "eps", "vd", "mgridref_y"), mode=mode, emb_dim=row["emb_dim"],
                                       nlayers=3, nn_arch=row["nn_arch"], device="cpu")
    assert un.layout == b["unflatten"].layout
    return dict(b, kind="mcd", params_flat=flat)


# ------------------------------------------------------------------------------------------ (b) box corners
def floored_grid(n):
    """mgridref_y of length n: every third entry at the floor 1e-3, one at 1.5, the rest 1.0."""
    m = np.ones(n, np.float32)
    m[1::3] = GRID_FLOOR
    m[2] = 1.5
    return m


HAIS_TARGETS = {"gmm": (2, 0.05, 2.0, 1.0)}     # (dim, eps, q's sigma, scale of q's mean) of tests/test_gpu_hais.py
_MANY40 = dict(dense=True, nbridges=40, init_sigma=15.0, grid="floored")
_UHA_SN = "MCD_CAIS_UHA_sn"

# `grad_eps`: the eps the GRADIENT comparisons of the case run at.  At eps = 1e-7 float32 alone moves d / d eps (and, at
# gamma = 1e-3, d / d gamma: eta_aux = gamma eps = 1e-10 under a square root) by more than GRAD_CAP of its scale, so such a
# gradient is no test of a kernel; the corner is moved inwards by decades until every leaf's float32 gap is below the cap.
# Worst leaf of the autograd oracle at float32 against float64, per decade (eps: gap):
#   eps-lo-gmm              1e-7: 6.4e-2 (eps)   1e-6: 1.7e-3
#   eps-lo-funnel           1e-7: 4.4e-2 (eps)   1e-6: 8.7e-2 (eps)   1e-5: 8.0e-3       (not monotone: the run at 1e-5 is kept)
#   eps-lo-dds40            1e-7: 0.76 (eps)     1e-6: 0.11           1e-5: 4.6e-2
#   eps-lo-var16            1e-7: 2.2e3 (eps)    1e-6: 92   1e-5: 2.8   1e-4: 7.8e-2   1e-3: 1.2e-3
#   gamma-lo-gmm-eps-lo     1e-7: 4.7e6 (gamma)  1e-6: 2.0e5   1e-5: 4.3e4   1e-4: 2.5e3   1e-3: 11   1e-2: 0.38   0.1: 1.7e-3
#   gamma-lo-funnel-eps-lo  1e-7: 4.9e5 (gamma)  1e-6: 1.0e5   1e-5: 1.0e4   1e-4: 1.5e2   1e-3: 14   1e-2: 8.9e-2 0.1: 4.2e-4
#   all-corners             1e-7: 6.4e5 (gamma)  1e-6: 7.3e4   1e-5: 2.7e4   1e-4: 4.2e2   1e-3: 3.5  1e-2: 0.12   0.1: 9.5e-4
# The forward comparisons stay on the face, eps = 1e-7.
CORNER_CASES = [
    # id, config, overrides, n0, mode
    ("eps-lo-gmm", "gmm_n300_k8", dict(dense=True, init_eps=EPS_LO, grad_eps=1e-6), 40, "MCD_CAIS_sn"),
    ("eps-lo-funnel", "funnel_n300_k64", dict(dense=True, nbridges=16, init_eps=EPS_LO, grad_eps=1e-5), 40, "MCD_CAIS_sn"),
    ("eps-lo-dds40", "many_gmm_n2000_k256_dds", dict(_MANY40, init_eps=EPS_LO, grad_eps=1e-5), 24, "MCD_CAIS_sn"),
    ("eps-lo-var16", "many_gmm_var_n16000_k256", dict(dense=True, nbridges=16, emb_dim=20, init_eps=EPS_LO, grad_eps=1e-3, grid="floored"),
     40,
     "MCD_CAIS_var_sn"),
    ("eps-hi-funnel", "funnel_n300_k64", dict(dense=True, nbridges=16, init_eps=EPS_HI), 40, "MCD_CAIS_sn"),
    ("eps-hi-dds40", "many_gmm_n2000_k256_dds", dict(_MANY40, init_eps=EPS_HI, eps_schedule=""), 24, "MCD_CAIS_sn"),
    ("gamma-lo-gmm", "gmm_n300_k8", dict(dense=True, init_eps=0.2, init_gamma=GAMMA_LO), 40, _UHA_SN),
    ("gamma-lo-gmm-eps-lo", "gmm_n300_k8", dict(dense=True, init_eps=EPS_LO, grad_eps=0.1, init_gamma=GAMMA_LO), 40, _UHA_SN),
    ("gamma-lo-funnel", "funnel_n300_k64", dict(dense=True, nbridges=8, init_eps=0.2, init_gamma=GAMMA_LO), 40, _UHA_SN),
    ("gamma-lo-funnel-eps-lo", "funnel_n300_k64", dict(dense=True, nbridges=8, init_eps=EPS_LO, grad_eps=0.1, init_gamma=GAMMA_LO), 40,
     _UHA_SN),
    # K = 8 on a grid of 9 entries: the bridges sit on the nodes, three of them at the end of a near-empty cell
    ("grid-gmm", "gmm_n300_k8", dict(dense=True, grid="floored"), 40, "MCD_CAIS_sn"),
    # every corner at once
    ("all-corners", "many_gmm_n2000_k256_dds", dict(_MANY40, init_eps=EPS_LO, grad_eps=0.1, init_gamma=GAMMA_LO), 24, _UHA_SN),
    # the dds clamp's neighbourhood: output layer x 1e5, so that four in ten network outputs lie between 1e3 and the clamp at
    # 1e4 and none beyond it (eps 1e-4 keeps the chain where it is)
    ("dds-near-clamp", "gmm_n300_k8", dict(dense=True, nn_arch="dds", init_eps=1e-4, out_scale=1e5), 40, "MCD_CAIS_sn"),
    # Hamiltonian AIS, K = 8 on a grid of 13 entries: bridges 1, 3, 5, 7 fall inside near-empty cells
    ("hais-grid", "hais:gmm", dict(nbridges=8, lfsteps=2, ngrid=12, grid="floored"), 40, "UHA"),
]

N0 = {c[0]: c[3] for c in CORNER_CASES}
N0.update({"gmm-cais": 40, "funnel-cais": 40, "many-dds": 24, "many-var": 40, "gmm-uha-sn": 40, "funnel-ula-sn": 40,
           "gmm-ula": 40, "funnel-uha": 40})

# seeds of parity_seeds(N0[id]) that the guard band drops (tests/test_oracle_trained_params.py re-derives them)
DROPPED = {}


def _seeds(cid):
    return tuple(s for s in range(1, N0[cid] + 1) if s not in DROPPED.get(cid, ()))


CASES = [(cid, None, {}, _seeds(cid), row["boundmode"]) for cid, row in TRAINED_ROWS.items()] + \
        [(cid, config, over, _seeds(cid), mode) for cid, config, over, _, mode in CORNER_CASES]
IDS = [c[0] for c in CASES]


def case_by_id(cid):
    return next(c for c in CASES if c[0] == cid)


def is_trained(case):
    return case[1] is None


def is_hais(case):
    return case[4] == "UHA"


def bridges_of(case):
    if is_trained(case):
        return TRAINED_ROWS[case[0]]["nbridges"]
    return case[2]["nbridges"] if "nbridges" in case[2] else synthetic.CONFIGS[case[1]]["nbridges"]


_BUILT = {}


def build_case(case, device="cpu", grad=False):
    """-> the built case: synthetic.build's dict plus kind = "mcd", or for mode "UHA" dict(kind = "hais", params_flat, unflatten,
    params_fixed = (dim, K, lfsteps), target_name).  Built once on the CPU and copied to `device`.  `grad`: the case as the
    gradient comparisons run it (eps = grad_eps where the case has one)."""
    cid, config, over, seeds, mode = case
    if grad and "grad_eps" in over:
        over = dict(over, init_eps=over["grad_eps"])
        cid = cid + "@grad"
    if cid not in _BUILT:
        if is_trained(case):
            flags, leaves = load_fixture(cid)
            assert flags == TRAINED_ROWS[cid], f"{cid}: the fixture was made with other flags than TRAINED_ROWS lists"
            b = initial_build(TRAINED_ROWS[cid])
            fill(b["params_flat"], b["unflatten"], leaves)
        elif is_hais(case):
            import hais_restatement as hr
            name = config.split(":")[1]
            dim, eps0, sigma0, mean_scale = HAIS_TARGETS[name]
            K, L = over["nbridges"], over["lfsteps"]
            flat, un, fixed = hr.make_params(dim, K, L, eps0, seed=K + 10 * L, mean_scale=mean_scale, sigma=sigma0,
                                             ngrid=over["ngrid"])
            b = dict(kind="hais", params_flat=flat, unflatten=un, params_fixed=fixed, target_name=name)
        else:
            over = {k: v for k, v in over.items() if k not in ("grid", "grad_eps")}
            b = dict(gc.build_case((cid, config, over, seeds, mode)), kind="mcd")
        if case[2].get("grid") == "floored":
            off, shape = next(v for p, v in b["unflatten"].layout.items() if p[1:] == ("mgridref_y",))
            b["params_flat"][off:off + shape[0]] = torch.from_numpy(floored_grid(shape[0]))
        _BUILT[cid] = b
    b = dict(_BUILT[cid])
    b["params_flat"] = b["params_flat"].to(device)
    return b


def leaf_value(b, *path):
    off, shape = next(v for p, v in b["unflatten"].layout.items() if p[1:] == path)
    n = 1
    for s in shape:
        n *= s
    return b["params_flat"][off:off + n].detach().cpu().numpy().reshape(shape)


def oracle_params(b):
    """The oracle's parameter dict (float64 NumPy); MCD_ULA keeps no network."""
    if b["kind"] == "hais":
        import hais_restatement as hr
        return hr.params_numpy(b["unflatten"], b["params_flat"])
    if b["params_fixed"][2] != "MCD_ULA":
        return synthetic.oracle_params(b["unflatten"], b["params_flat"])
    train, notrain = b["unflatten"](b["params_flat"].detach().cpu())
    allp = {**train, **notrain}
    f = lambda t: np.asarray(t.numpy(), np.float64)
    return {"vd": {k: f(v) for k, v in allp["vd"].items()}, "eps": f(allp["eps"]), "gamma": f(allp["gamma"]),
            "mgridref_y": f(allp["mgridref_y"]), "gridref_x": f(allp["gridref_x"]), "target_x": f(allp["target_x"])}


def _arch(b):
    spec = b["params_fixed"][3]
    return "dds" if spec is None else spec.arch


def flat_gradient(b, g):
    """The oracle's gradient dict re-assembled in params_flat order (float64); leaves it does not hold stay zero."""
    un = b["unflatten"]
    flat = torch.zeros(b["params_flat"].numel(), dtype=torch.float64)
    by_path = {path[1:]: v for path, v in un.layout.items()}

    def put(path, val):
        off, shape = by_path[path]
        a = np.asarray(val, np.float64).reshape(-1)
        flat[off:off + a.size] = torch.from_numpy(a)
    if b["kind"] == "hais":
        for path, val in g.items():
            put(path, val)
        return flat
    for path in (("vd", "mean"), ("vd", "logdiag"), ("eps",), ("mgridref_y",), ("gamma",)):
        node = g
        for k in path:
            node = node.get(k) if isinstance(node, dict) else None
            if node is None:
                break
        if node is not None:
            put(path, node)
    gs = g.get("sn")
    if gs is None:
        return flat
    if "W1" in gs:
        for i, (wk, bk) in enumerate((("W1", "b1"), ("W2", "b2"), ("W3", "b3"))):
            put(("sn", "nn", i, 0), gs[wk])
            put(("sn", "nn", i, 1), gs[bk])
        put(("sn", "emb"), gs["emb"])
        put(("sn", "factor_sn"), gs["factor_sn"])
    else:
        put(("sn", "drift_net", "timestep_phase"), gs["timestep_phase"])
        for mod, (wk, bk) in (("linear", ("t_w1", "t_b1")), ("linear_1", ("t_w2", "t_b2")), ("linear_2", ("s_w1", "s_b1")),
                              ("linear_3", ("s_w2", "s_b2")), ("linear_zero", ("s_w3", "s_b3"))):
            put(("sn", "drift_net/~/" + mod, "w"), gs[wk])
            put(("sn", "drift_net/~/" + mod, "b"), gs[bk])
    return flat


def forward_oracle(b, seeds, dtype=np.float64, trace=None):
    """-> (losses, z) of the NumPy oracle (mcd) or the restatement's forward (hais) in `dtype`."""
    seeds = np.asarray(seeds, np.int32)
    if b["kind"] == "hais":
        import hais_restatement as hr
        dim, K, L = b["params_fixed"]
        l, z = hr.forward(seeds, oracle_params(b), dim, K, L, b["target_name"], trace=trace,
                          dtype=torch.float64 if dtype == np.float64 else torch.float32)
        return np.asarray(l, np.float64), np.asarray(z, np.float64)
    from helpers import oracle_target
    cfg = b["cfg"]
    dim, K, mode, _ = b["params_fixed"]
    l, z = orc.compute_log_elbo_batch(seeds, oracle_params(b), dim, K, mode, _arch(b), oracle_target(cfg),
                                      eps_schedule=cfg["eps_schedule"], grad_clipping=cfg["grad_clipping"], dtype=dtype,
                                      trace=trace)
    return np.asarray(l, np.float64), np.asarray(z, np.float64)


def grad_oracle(b, seeds, dtype=torch.float64, trace=None):
    """-> (losses, z, flat gradient) of the autograd oracle in `dtype`, all float64 NumPy / torch."""
    seeds = np.asarray(seeds, np.int32)
    if b["kind"] == "hais":
        import hais_restatement as hr
        dim, K, L = b["params_fixed"]
        l, z, g = hr.bound_and_grad(seeds, oracle_params(b), dim, K, L, b["target_name"], dtype=dtype)
        return np.asarray(l, np.float64), np.asarray(z, np.float64), flat_gradient(b, g)
    cfg = b["cfg"]
    dim, K, mode, _ = b["params_fixed"]
    _, l, z, g = ot.bound_and_grad(seeds, oracle_params(b), dim, K, mode, _arch(b), cfg["model"], cfg["eps_schedule"],
                                   cfg["grad_clipping"], trace=trace, dtype=dtype)
    return l, z, flat_gradient(b, g)


# ------------------------------------------------------------------------------------------ seeds
def thresholds(b):
    if b["kind"] == "hais":
        return {"lp": -gc.FLOOR} if b["target_name"] == "many_gmm" else {}
    if b["params_fixed"][3] is None:          # MCD_ULA: no network, no clip
        return {"lp": -gc.FLOOR} if b["cfg"]["model"] == "many_gmm" else {}
    return gc.thresholds(b)


def select_seeds(case):
    """The survivors of parity_seeds(N0[id]): a particle whose own chain comes within gated_cases.DELTA (relative) of a
    threshold it is compared with is dropped."""
    n0 = N0[case[0]]
    seeds = synthetic.parity_seeds(n0)
    bad = np.zeros(n0, bool)
    for grad in ((False, True) if "grad_eps" in case[2] else (False,)):      # under both parameter sets of the case
        b = build_case(case, grad=grad)
        th = thresholds(b)
        if not th:
            continue
        trace = {}
        if b["kind"] == "hais":
            forward_oracle(b, seeds, trace=trace)
        else:
            grad_oracle(b, seeds, trace=trace)
        for key, thr in th.items():
            a = np.abs(gc._stack(trace, key))
            bad |= (np.abs(a - thr) <= gc.DELTA * thr).any(axis=(0, 2))
    return tuple(int(s) for s in seeds[~bad])


# ------------------------------------------------------------------------------------------ the float32 gap and the bars
LOSS_METRICS = ("mean", "lnz", "rel_p99", "rel_max", "z_p99", "z_max")


def loss_metrics(l, l_ref, z, z_ref):
    """The six quantities helpers.compare_losses bounds, each in the unit of its bar: mean and ln Z error over
    max(1, |reference|), p99 and worst relative loss error, p99 and worst |z - z_ref| over z_scale.  -> (dict, z_scale)"""
    l, l_ref = np.asarray(l, np.float64), np.asarray(l_ref, np.float64)
    z = np.asarray(z, np.float64).reshape(len(l_ref), -1)
    z_ref = np.asarray(z_ref, np.float64).reshape(len(l_ref), -1)
    f = np.isfinite(l_ref)
    rel = np.abs(l[f] - l_ref[f]) / np.maximum(1.0, np.abs(l_ref[f]))
    zerr = np.abs(z - z_ref)[f]
    z_scale = max(1.0, float(np.quantile(np.abs(z_ref[f]), 0.99)))
    return {"mean": abs(l[f].mean() - l_ref[f].mean()) / max(1.0, abs(l_ref[f].mean())),
            "lnz": abs(orc.ln_z(l) - orc.ln_z(l_ref)) / max(1.0, abs(orc.ln_z(l_ref))),
            "rel_p99": float(np.quantile(rel, 0.99)), "rel_max": float(rel.max()),
            "z_p99": float(np.quantile(zerr, 0.99)) / z_scale, "z_max": float(zerr.max()) / z_scale}, z_scale


def standard_loss_bars(K):
    """helpers.compare_losses' defaults (z_max: asserted for K <= 32 only)."""
    return {"mean": 1e-3, "lnz": 1e-3, "rel_p99": 5e-3, "rel_max": 1e-3 if K <= 32 else 0.2, "z_p99": 1e-3, "z_max": 1e-3}


def forward_gap32(case):
    """loss_metrics of the oracle at float32 against float64 on the case's seeds; the +inf sets must coincide."""
    b = build_case(case)
    l64, z64 = forward_oracle(b, case[3], np.float64)
    l32, z32 = forward_oracle(b, case[3], np.float32)
    assert np.array_equal(np.isinf(l32), np.isinf(l64)), (case[0], "the +inf sets of float32 and float64 differ")
    return loss_metrics(l32, l64, z32, z64)[0]


def leaf_name(path):
    """Layout key (group, *path) -> "vd/mean", "sn/nn/0/0", ...: the key of GRAD_GAP32 and of `_compare`'s per-leaf tol."""
    return "/".join(map(str, path[1:]))


def leaf_errors(un, g, g_ref):
    """{leaf name: max |g - g_ref| / max |g_ref|} over the leaves whose reference is not identically zero."""
    out = {}
    for path, (off, shape) in un.layout.items():
        numel = max(1, int(np.prod(shape)))
        a, r = g[off:off + numel], g_ref[off:off + numel]
        scale = float(r.abs().max())
        if scale > 0:
            out[leaf_name(path)] = float((a - r).abs().max()) / scale
    return out


def grad_gap32(case):
    b = build_case(case, grad=True)
    g64 = grad_oracle(b, case[3])[2]
    g32 = grad_oracle(b, case[3], dtype=torch.float32)[2]
    return leaf_errors(b["unflatten"], g32, g64)


QUARTER = 0.25           # a case keeps the suite's standard bar while its stored gap is at most this share of it
FACTOR = 4.0             # otherwise the bar is this multiple of the gap
GRAD_CAP = 5e-2          # a leaf whose float32 gap exceeds this share of its scale is no test of the kernel on that leaf
GRAD_LISTED = 2e-4       # GRAD_GAP32 lists the leaves whose gap is above this; every other leaf is asserted below 1.5 x it


def loss_bars(cid, K):
    """{metric: bar} in the metric's unit: the standard bar, or FACTOR x the stored float32 gap where that gap is more than a
    quarter of the standard bar."""
    std = standard_loss_bars(K)
    gap = LOSS_GAP32[cid]
    return {m: (std[m] if gap[m] <= QUARTER * std[m] else FACTOR * gap[m]) for m in LOSS_METRICS}


def grad_tols(cid):
    """{leaf name: bar} for the leaves on a loosened bar (every other leaf: gated_cases.BAR)."""
    return {leaf: FACTOR * g for leaf, g in GRAD_GAP32.get(cid, {}).items() if g > QUARTER * gc.BAR}


# Measured by tests/test_oracle_trained_params.py (which fails when a recomputed value exceeds 1.5 x the stored one): the NumPy
# oracle / the restatement at float32 against float64 on the case's seeds, in the units of loss_metrics.
LOSS_GAP32 = {
    "gmm-cais": {"mean": 8.9e-07, "lnz": 1.7e-06, "rel_p99": 6.4e-06, "rel_max": 6.5e-06, "z_p99": 2.2e-07, "z_max":
        2.4e-07},
    "funnel-cais": {"mean": 1.2e-06, "lnz": 1.5e-07, "rel_p99": 1.9e-05, "rel_max": 2.2e-05, "z_p99": 2.3e-07, "z_max":
        9.8e-07},
    "many-dds": {"mean": 3.4e-06, "lnz": 1.0e-04, "rel_p99": 1.9e-04, "rel_max": 2.3e-04, "z_p99": 1.5e-07, "z_max":
        1.7e-07},
    "many-var": {"mean": 1.0e-07, "lnz": 1.5e-05, "rel_p99": 7.8e-06, "rel_max": 1.0e-05, "z_p99": 9.2e-08, "z_max":
        9.7e-08},
    "gmm-uha-sn": {"mean": 9.3e-07, "lnz": 1.5e-07, "rel_p99": 4.6e-06, "rel_max": 5.8e-06, "z_p99": 5.2e-07, "z_max":
        1.7e-06},
    "funnel-ula-sn": {"mean": 1.7e-07, "lnz": 1.4e-07, "rel_p99": 5.9e-06, "rel_max": 6.2e-06, "z_p99": 2.1e-07, "z_max":
        2.6e-07},
    "gmm-ula": {"mean": 2.3e-07, "lnz": 5.1e-07, "rel_p99": 3.4e-06, "rel_max": 3.6e-06, "z_p99": 1.7e-07, "z_max":
        1.7e-07},
    "funnel-uha": {"mean": 8.1e-07, "lnz": 7.2e-07, "rel_p99": 6.5e-06, "rel_max": 6.6e-06, "z_p99": 2.3e-07, "z_max":
        5.0e-07},
    "eps-lo-gmm": {"mean": 1.9e-05, "lnz": 1.3e-04, "rel_p99": 8.2e-04, "rel_max": 8.4e-04, "z_p99": 1.5e-07, "z_max":
        1.6e-07},
    "eps-lo-funnel": {"mean": 1.7e-05, "lnz": 1.8e-03, "rel_p99": 3.9e-03, "rel_max": 4.1e-03, "z_p99": 2.5e-07, "z_max":
        3.9e-07},
    "eps-lo-dds40": {"mean": 4.1e-05, "lnz": 7.6e-05, "rel_p99": 6.3e-04, "rel_max": 6.6e-04, "z_p99": 5.6e-07, "z_max":
        6.1e-07},
    "eps-lo-var16": {"mean": 1.2e-05, "lnz": 1.5e-04, "rel_p99": 1.0e-03, "rel_max": 1.1e-03, "z_p99": 2.0e-07, "z_max":
        2.2e-07},
    "eps-hi-funnel": {"mean": 2.1e-07, "lnz": 2.9e-07, "rel_p99": 8.9e-06, "rel_max": 1.0e-05, "z_p99": 1.6e-07, "z_max":
        2.3e-07},
    "eps-hi-dds40": {"mean": 2.1e-07, "lnz": 3.1e-06, "rel_p99": 2.0e-05, "rel_max": 2.1e-05, "z_p99": 5.6e-08, "z_max":
        6.7e-08},
    "gamma-lo-gmm": {"mean": 1.0e-06, "lnz": 1.7e-05, "rel_p99": 6.0e-05, "rel_max": 7.6e-05, "z_p99": 1.2e-06, "z_max":
        1.4e-06},
    "gamma-lo-gmm-eps-lo": {"mean": 6.2e-06, "lnz": 2.8e-05, "rel_p99": 4.6e-05, "rel_max": 5.2e-05, "z_p99": 1.5e-07,
        "z_max": 2.1e-07},
    "gamma-lo-funnel": {"mean": 4.7e-06, "lnz": 1.1e-06, "rel_p99": 1.4e-04, "rel_max": 1.5e-04, "z_p99": 1.3e-07, "z_max":
        1.7e-07},
    "gamma-lo-funnel-eps-lo": {"mean": 5.2e-06, "lnz": 6.2e-05, "rel_p99": 1.4e-04, "rel_max": 1.6e-04, "z_p99": 1.5e-07,
        "z_max": 2.0e-07},
    "grid-gmm": {"mean": 4.9e-07, "lnz": 1.0e-06, "rel_p99": 3.3e-06, "rel_max": 3.8e-06, "z_p99": 1.7e-07, "z_max":
        1.9e-07},
    "all-corners": {"mean": 1.9e-07, "lnz": 2.4e-05, "rel_p99": 6.1e-05, "rel_max": 7.5e-05, "z_p99": 1.7e-07, "z_max":
        1.7e-07},
    "dds-near-clamp": {"mean": 1.9e-07, "lnz": 2.4e-08, "rel_p99": 6.3e-07, "rel_max": 6.8e-07, "z_p99": 1.7e-07, "z_max":
        1.9e-07},
    "hais-grid": {"mean": 1.1e-07, "lnz": 4.3e-08, "rel_p99": 1.6e-06, "rel_max": 1.9e-06, "z_p99": 1.7e-07, "z_max":
        2.4e-07},
}
# The same for the autograd oracle's gradient: {case: {leaf name: max |g32 - g64| / max |g64|}}, leaves above GRAD_LISTED only.
GRAD_GAP32 = {
    "eps-lo-gmm": {"eps": 1.8e-03},
    "eps-lo-funnel": {"eps": 8.4e-03},
    "eps-lo-dds40": {"eps": 4.9e-02, "mgridref_y": 2.2e-04, "sn/drift_net/~/linear/w": 2.5e-04, "sn/drift_net/~/linear_2/w":
        2.6e-04},
    "eps-lo-var16": {"eps": 1.3e-03, "vd/logdiag": 4.5e-04},
    "eps-hi-dds40": {"eps": 8.2e-04, "mgridref_y": 5.3e-04, "sn/drift_net/timestep_phase": 2.7e-04,
        "sn/drift_net/~/linear/w": 2.3e-04, "sn/drift_net/~/linear_3/w": 3.5e-04, "sn/drift_net/~/linear_zero/w": 2.6e-04,
        "vd/logdiag": 6.1e-04, "vd/mean": 4.1e-04},
    "gamma-lo-gmm-eps-lo": {"gamma": 1.8e-03},
    "gamma-lo-funnel": {"gamma": 1.1e-03},
    "gamma-lo-funnel-eps-lo": {"gamma": 4.4e-04, "sn/factor_sn": 3.5e-04},
    "all-corners": {"gamma": 1.0e-03},
}
