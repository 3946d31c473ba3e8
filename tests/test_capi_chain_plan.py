"""The C host path of the reverse and segment entry points (csrc/cmcd_api.hip: chain_call_begin, ldvi_call_begin,
hais_chain_begin), on the CPU: every call here is refused before any GPU work, with dummy pointers that are never followed.

tests/golden/capi_chain_refusals.json holds what the library answered BEFORE these entry points were given one preamble per
family (commit 7ce2fb7): the size queries of all eight reverse / segment entry points and of cmcd_ldvi_bound_grad over a grid,
with the reason of every zero, and the (return code, message) pairs of a fixed sequence of refused calls — every single fault
the test_capi_* files use, then calls with two and three faults at once, which is what pins the ORDER of the refusals.  It was
written from that commit's library with

    CMCD_LIB_PATH=<that commit's libcmcd_hip.so> python -c "import sys; sys.path.insert(0, 'tests'); \
        import test_capi_chain_plan as t; t.write_fixture()"

and is not to be regenerated from the library under test."""
import ctypes as C
import json
import os

import pytest

from cmcd_amd import _lib, hais, ldvi
from cmcd_amd import mcdboundingmachine as mcdbm
from cmcd_amd import synthetic
from test_capi_plan import NETS

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "capi_chain_refusals.json")
NS = (1, 16, 17, 300, 2000)
PTR = 4096      # a non-null, 16-byte aligned address nobody dereferences
GMM, FUNNEL, MANY, LGCP = 0, 1, 2, 3
INTS = ("n", "n_params", "n_consts", "ws_bytes", "k0", "k1", "use_net", "target", "dim", "K", "L")
# the argument lists of include/cmcd_hip.h; `hlay` is a cmcd_hais_layout, every other name outside INTS a pointer
_DESC = "desc lay"
_TAIL = "params n_params consts n_consts ws ws_bytes"
SIG = {
    "cmcd_bound_reverse": f"{_DESC} seeds x n {_TAIL} w z0 stats stream",
    "cmcd_bound_reverse_uha": f"{_DESC} seeds x n {_TAIL} w z0 rho0 stats stream",
    "cmcd_bound_segment": f"{_DESC} k0 k1 seeds n {_TAIL} z wpath key lg stats stream",
    "cmcd_bound_segment_uha": f"{_DESC} k0 k1 seeds n {_TAIL} z rho wpath key lg stats stream",
    "cmcd_ldvi_bound_grad": f"{_DESC} use_net seeds n params n_params consts n_consts omega ws ws_bytes loss z stats grad stream",
    "cmcd_bound_reverse_ldvi": f"{_DESC} use_net seeds x n {_TAIL} w z0 rho0 stats stream",
    "cmcd_bound_segment_ldvi": f"{_DESC} use_net k0 k1 seeds n {_TAIL} z rho wpath key lg stats stream",
    "cmcd_bound_reverse_hais": f"target dim K L hlay seeds x n {_TAIL} w z0 rho0 stats stream",
    "cmcd_bound_segment_hais": f"target dim K L hlay k0 k1 seeds n {_TAIL} z rho wpath key lg stats stream",
}
DESC_QUERIES = ("cmcd_reverse_workspace_bytes", "cmcd_reverse_uha_workspace_bytes", "cmcd_segment_workspace_bytes",
                "cmcd_segment_uha_workspace_bytes")
LDVI_QUERIES = ("cmcd_reverse_ldvi_workspace_bytes", "cmcd_segment_ldvi_workspace_bytes")
HAIS_QUERIES = ("cmcd_reverse_hais_workspace_bytes", "cmcd_segment_hais_workspace_bytes")


def _edit(desc, **kw):
    return _lib.Desc(**{**{k: getattr(desc, k) for k, _ in _lib.Desc._fields_}, **kw})


def _answer(nb):
    return [nb, "" if nb else _lib.last_error()]      # a zero answer comes with its reason


def _sizes(L):
    out = {}
    for name, target, dim, arch, emb, K in NETS:
        for mode in range(5):
            d = _lib.Desc(dim=dim, nbridges=K, mode=mode, arch=arch, emb_dim=emb, target=target, eps_schedule=2, grad_clipping=1,
                          ngrid=8, reserved=0)
            out[f"{name}/mode{mode}"] = [[n] + [a for q in DESC_QUERIES for a in _answer(getattr(L, q)(C.byref(d), n))] for n in NS]
        d = _lib.Desc(dim=dim, nbridges=K, mode=0, arch=arch, emb_dim=emb, target=target, eps_schedule=0, grad_clipping=0, ngrid=8,
                      reserved=0)
        for use_net in (0, 1):
            out[f"{name}/ldvi/use_net{use_net}"] = [
                [n] + [a for q in LDVI_QUERIES for a in _answer(getattr(L, q)(C.byref(d), use_net, n))]
                + [a for g in (0, 1) for a in _answer(L.cmcd_ldvi_workspace_bytes(C.byref(d), use_net, n, g))] for n in NS]
        for lf in (1, 3):
            out[f"{name}/hais/lfsteps{lf}"] = [[n] + [a for q in HAIS_QUERIES for a in _answer(getattr(L, q)(target, dim, K, lf, n))]
                                               for n in NS]
    return out


def _call(lib, entry, defaults, null=(), **kw):
    """One call with dummy pointers and workspace_bytes = 0 unless told otherwise -> [return code, cmcd_last_error]."""
    v = dict(defaults, **kw)
    args = []
    for tok in SIG[entry].split():
        if tok in INTS:
            args.append(v[tok])
        elif tok == "omega":
            args.append(C.c_float(1.0))
        elif tok == "stream" or tok in null:
            args.append(None)
        elif tok in ("desc", "lay"):
            args.append(C.byref(v[tok]))
        elif tok == "hlay":
            args.append(v["lay"])
        elif tok == "consts":
            args.append(PTR if v["n_consts"] else None)
        else:
            args.append(v.get("ws_ptr", PTR) if tok == "ws" else PTR)
    rc = getattr(lib, entry)(*args)
    assert rc != 0, (entry, null, kw)      # nothing here may reach a launch
    return [rc, _lib.last_error()]


def _setups():
    """entry -> the arguments of a call that is valid but for its empty workspace (gmm, K = 8, n = 33)."""
    out = {}
    base = dict(n=33, n_consts=0, ws_bytes=0, k0=0, k1=2)
    for entries, over in ((("cmcd_bound_reverse", "cmcd_bound_segment"), {}),
                          (("cmcd_bound_reverse_uha", "cmcd_bound_segment_uha"), dict(boundmode="MCD_CAIS_UHA_sn"))):
        b = synthetic.build("gmm_n300_k8", device="cpu", **over)
        plan = mcdbm._plan(b["unflatten"], b["params_fixed"], b["target"], b["eps_schedule"], b["grad_clipping"])
        for e in entries:
            out[e] = dict(base, desc=plan.desc, lay=plan.lay, n_params=b["params_flat"].numel())
    from cmcd_amd.model_handler import load_model
    flat, un, fixed = ldvi.initialize(2, nbridges=8, eps=0.01, emb_dim=20, mode="MCD_U_a-lp-sn", nn_arch="geffner", device="cpu",
                                      trainable=("eta", "gamma", "eps", "vd", "mgridref_y"))
    desc, lay, use_net = ldvi._plan(un, fixed, load_model("gmm")[0])
    for e in ("cmcd_ldvi_bound_grad", "cmcd_bound_reverse_ldvi", "cmcd_bound_segment_ldvi"):
        out[e] = dict(base, desc=desc, lay=lay, use_net=use_net, n_params=flat.numel())
    flat, un, _ = hais.initialize(dim=2, nbridges=8, lfsteps=1, eps=0.05, eta=0.5, device="cpu",
                                  trainable=("eta", "eps", "vd", "mgridref_y"))
    for e in ("cmcd_bound_reverse_hais", "cmcd_bound_segment_hais"):
        out[e] = dict(base, target=GMM, dim=2, K=8, L=1, lay=hais._layout(un), n_params=flat.numel())
    return out


def _faults(entry, d):
    """(name, null pointers, changed arguments): the single faults, then two and three at once."""
    seg, uha_boundmode, is_ldvi = "segment" in entry, entry.endswith("_hais"), "ldvi" in entry
    ptrs = [t for t in SIG[entry].split() if t not in INTS + ("omega", "stream", "consts", "desc")]
    many = dict(target=MANY) if uha_boundmode else dict(desc=_edit(d["desc"], target=MANY))
    bad_range = dict(k0=3, k1=2) if seg else {}
    F = [(f"null {p}", (p,), {}) for p in ptrs]
    F += [("n = 0", (), dict(n=0)), ("n = -5", (), dict(n=-5)), ("n above 2^31", (), dict(n=(1 << 31) + 1))]
    if seg:
        F += [("k0 = -1", (), dict(k0=-1)), ("k0 = k1", (), dict(k0=2, k1=2)), ("k0 > k1", (), dict(k0=3, k1=2)),
              ("k1 = K + 1", (), dict(k1=9)), ("k0 = K", (), dict(k0=8, k1=9)), ("no seeds past bridge 0", ("seeds",), dict(k0=1)),
              ("the last bridge alone", (), dict(k0=7, k1=8)), ("null rho past bridge 0", ("rho",), dict(k0=1)),
              ("null z past bridge 0", ("z",), dict(k0=1))]
    F += [("layout outside params_flat", (), dict(n_params=10)), ("layout outside by one", (), dict(n_params=d["n_params"] - 1)),
          ("many_gmm without constants", (), many), ("many_gmm bad count", (), dict(many, n_consts=4)),
          ("many_gmm even count", (), dict(many, n_consts=80)), ("many_gmm 65 mixtures", (), dict(many, n_consts=131)),
          ("many_gmm null constants", ("consts",), dict(many, n_consts=81)),
          ("many_gmm short workspace, 40 mixtures", (), dict(many, n_consts=81)),
          ("many_gmm short workspace, 64 mixtures", (), dict(many, n_consts=129)),
          ("short workspace", (), {}), ("short workspace, 64 bytes", (), dict(ws_bytes=64)),
          ("short workspace, n = 2000", (), dict(n=2000)),
          ("unaligned workspace", (), dict(ws_ptr=24, ws_bytes=1 << 40))]
    if uha_boundmode:
        lay = d["lay"]
        grid = lambda g: _lib.HaisLayout(**dict({k: getattr(lay, k) for k in _lib.HAIS_LAYOUT_FIELDS}, ngrid=g))
        F += [("K = 0", (), dict(K=0)), ("K = -3", (), dict(K=-3)), ("L = 0", (), dict(L=0)), ("K = 4097", (), dict(K=4097)),
              ("K * L above 2^24", (), dict(K=4096, L=4097)), ("lgcp", (), dict(target=LGCP, dim=1600)), ("dim = 3", (), dict(dim=3)),
              ("dim = 0", (), dict(dim=0)), ("funnel at dim 2", (), dict(target=FUNNEL)), ("target 7", (), dict(target=7)),
              ("ngrid = 2000", (), dict(lay=grid(2000))), ("ngrid = -1", (), dict(lay=grid(-1))),
              # two and three at once
              ("a null pointer and K = 0", (ptrs[2],), dict(K=0)), ("K = 0 and n = 0", (), dict(K=0, n=0)),
              ("n = 0 and lgcp", (), dict(n=0, target=LGCP, dim=1600)), ("lgcp and K = 0", (), dict(target=LGCP, dim=1600, K=0)),
              ("no instance and K above its cap", (), dict(dim=3, K=4097)), ("K above its cap and a bad range", (), dict(K=4097, **bad_range)),
              ("n = 0 and a bad range", (), dict(n=0, **bad_range)), ("a bad range and ngrid = 2000", (), dict(lay=grid(2000), **bad_range)),
              ("ngrid = 2000 and a layout outside", (), dict(lay=grid(2000), n_params=10)),
              ("a bad range and a layout outside", (), dict(n_params=10, **bad_range)),
              ("a layout outside and many_gmm without constants", (), dict(many, n_params=10)),
              ("lgcp, everything else null", tuple(ptrs), dict(target=LGCP, dim=1600)),
              ("null stats, n = 0 and a bad range", ("stats",), dict(n=0, **bad_range)),
              ("n = 0, a bad range and a layout outside", (), dict(n=0, n_params=10, **bad_range)),
              ("a bad range, a layout outside and constants missing", (), dict(many, n_params=10, **bad_range))]
        return F
    desc = d["desc"]
    other = 0 if desc.mode == 4 else 4      # MCD_CAIS_sn for the 2nd-order calls, MCD_CAIS_UHA_sn for the overdamped ones
    F += [("null desc", ("desc",), {}), ("mode 7", (), dict(desc=_edit(desc, mode=7))),
          ("the other family's mode", (), dict(desc=_edit(desc, mode=other))),
          ("lgcp", (), dict(desc=_edit(desc, target=LGCP, dim=1600))), ("no instance", (), dict(desc=_edit(desc, emb_dim=200))),
          ("134 wide", (), dict(desc=_edit(desc, emb_dim=130))), ("dds", (), dict(desc=_edit(desc, arch=1, emb_dim=64))),
          ("nbridges = 0", (), dict(desc=_edit(desc, nbridges=0))), ("nbridges = 5000", (), dict(desc=_edit(desc, nbridges=5000))),
          ("ngrid = 40", (), dict(desc=_edit(desc, ngrid=40)))]
    if is_ldvi:
        F += [("without the network", (), dict(use_net=0)), ("without the network, lgcp", (), dict(use_net=0, desc=_edit(desc, target=LGCP, dim=1600))),
              ("without the network, layout outside", (), dict(use_net=0, n_params=10)),
              ("without the network, funnel at dim 4", (), dict(use_net=0, desc=_edit(desc, target=FUNNEL, dim=4))),
              ("gamma leaf missing", (), dict(lay=_lib.Layout(**dict({k: getattr(d["lay"], k) for k in _lib.LAYOUT_FIELDS}, gamma=-1)))),
              ("without the network, gamma leaf outside", (),
               dict(use_net=0, lay=_lib.Layout(**dict({k: getattr(d["lay"], k) for k in _lib.LAYOUT_FIELDS}, gamma=d["n_params"]))))]
    # two and three at once
    F += [("null params and n = 0", ("params",), dict(n=0)), ("null stats and a layout outside", ("stats",), dict(n_params=10)),
          ("n = 0 and a bad range", (), dict(n=0, **bad_range)), ("n = 0 and a layout outside", (), dict(n=0, n_params=10)),
          ("a bad range and a layout outside", (), dict(n_params=10, **bad_range)),
          ("a bad range and the other family's mode", (), dict(desc=_edit(desc, mode=other), **bad_range)),
          ("no instance and a layout outside", (), dict(desc=_edit(desc, emb_dim=200), n_params=10)),
          ("a layout outside and many_gmm without constants", (), dict(many, n_params=10)),
          ("many_gmm bad count and 64 bytes", (), dict(many, n_consts=4, ws_bytes=64)),
          ("mode 7, everything else null", tuple(ptrs), dict(desc=_edit(desc, mode=7))),
          ("lgcp, everything else null", tuple(ptrs), dict(desc=_edit(desc, target=LGCP, dim=1600), n=0)),
          ("null desc, everything else null", ("desc",) + tuple(ptrs), dict(n=0)),
          ("null stats, n = 0 and a bad range", ("stats",), dict(n=0, **bad_range)),
          ("n = 0, a bad range and a layout outside", (), dict(n=0, n_params=10, **bad_range)),
          ("a bad range, a layout outside and constants missing", (), dict(many, n_params=10, **bad_range)),
          ("a layout outside, constants missing and 64 bytes", (), dict(many, n_params=10, ws_bytes=64))]
    return F


def _refusals(L):
    out = {}
    for entry, d in _setups().items():
        out[entry] = [[name] + _call(L, entry, d, null, **kw) for name, null, kw in _faults(entry, d)]
    return out


def write_fixture():
    L = _lib.lib()
    with open(FIXTURE, "w") as f:
        json.dump({"library": "7ce2fb7", "sizes": _sizes(L), "refusals": _refusals(L)}, f, indent=0, sort_keys=True)


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE) as f:
        return json.load(f)


def _first_difference(got, want):
    assert list(got) == sorted(want), (sorted(set(got) ^ set(want)))
    for key in got:
        assert len(got[key]) == len(want[key]), (key, len(got[key]), len(want[key]))
        for row, stored in zip(got[key], want[key]):
            assert row == stored, (key, row, stored)


def test_size_queries_reproduce_the_stored_answers(hip_lib, golden):
    got = _sizes(hip_lib)
    _first_difference(dict(sorted(got.items())), golden["sizes"])
    flat = [r for rows in got.values() for r in rows]
    assert len(got) == len(NETS) * 9 and any(r[1] == 0 for r in flat) and any(r[1] > 0 and r[3] > 0 for r in flat)


def test_entry_points_refuse_bad_input_in_the_stored_order(hip_lib, golden):
    got = _refusals(hip_lib)
    assert set(got) == set(SIG)
    _first_difference(dict(sorted(got.items())), golden["refusals"])
    for entry, rows in got.items():
        texts = " | ".join(r[2] for r in rows)
        for text in ("null pointer", "out of range", "layout offset", "many_gmm needs", "workspace too small", "lgcp"):
            assert text in texts, (entry, text)
        assert ("0 <= k0 < k1" in texts and "needs seeds" in texts) == ("segment" in entry), entry
