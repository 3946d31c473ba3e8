"""The C host path's workspace plan (csrc/cmcd_api.hip: CallPlan), on the CPU: every call here is refused before any GPU work.

tests/golden/capi_workspace_sizes.json holds what the library answered BEFORE the entry points were split from the kernels
and given one plan (commit f4eb563): the three size queries over a grid, the byte count each entry point demands of a short
workspace, and the (return code, message) pairs of a fixed sequence of refused calls.  It was written from that commit's
library with

    CMCD_LIB_PATH=<that commit's libcmcd_hip.so> python -c "import sys; sys.path.insert(0, 'tests'); \
        import test_capi_plan as t; t.write_fixture()"

and is not to be regenerated from the library under test."""
import ctypes as C
import json
import os
import re

import pytest

from cmcd_amd import _lib
from cmcd_amd import mcdboundingmachine as mcdbm
from cmcd_amd import synthetic

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "capi_workspace_sizes.json")
NS = (1, 20, 224, 225, 300, 2000, 2048, 2049, 16000)
# (name, target, dim, arch, emb_dim, nbridges): the widths the suite runs — geffner 2 + 20 = 22, 10 + 48 = 58, 2 + 130 = 132, their
# 2nd-order forms on concat(z, rho) (24, 68, 134), the dds net, and lgcp d = 1600
NETS = (("gmm_w22", 0, 2, 0, 20, 8), ("gmm_dds", 0, 2, 1, 20, 8), ("funnel_w58", 1, 10, 0, 48, 64), ("funnel_dds", 1, 10, 1, 20, 64),
        ("many_gmm_w22", 2, 2, 0, 20, 256), ("many_gmm_w132", 2, 2, 0, 130, 256), ("many_gmm_dds", 2, 2, 1, 20, 256),
        ("lgcp_d1600", 3, 1600, 0, 20, 128))
QUERIES = ("cmcd_workspace_bytes", "cmcd_grad_workspace_bytes", "cmcd_bound_grad_workspace_bytes")
FORWARD_LIKE = ("cmcd_bound_forward", "cmcd_bound_forward_prepared", "cmcd_bound_var_forward")
VAR_GRADS = ("cmcd_bound_var_grad", "cmcd_bound_var_grad_kept")
ENTRIES = FORWARD_LIKE + ("cmcd_bound_grad",) + VAR_GRADS
QUERY_OF = {"cmcd_bound_forward": QUERIES[0], "cmcd_bound_forward_prepared": QUERIES[0], "cmcd_bound_var_forward": QUERIES[1],
            "cmcd_bound_var_grad": QUERIES[1], "cmcd_bound_var_grad_kept": QUERIES[1], "cmcd_bound_grad": QUERIES[2]}
PTR = 4096      # a non-null, 16-byte aligned address nobody dereferences: workspace_bytes = 0 refuses every call before a launch


def _sizes(L):
    out = {}
    for name, target, dim, arch, emb, K in NETS:
        for mode in range(5):
            d = _lib.Desc(dim=dim, nbridges=K, mode=mode, arch=arch, emb_dim=emb, target=target, eps_schedule=2,
                          grad_clipping=1, ngrid=8, reserved=0)
            rows = []
            for n in NS:
                row = [n]
                for q in QUERIES:
                    nb = getattr(L, q)(C.byref(d), n)
                    row += [nb, "" if nb else _lib.last_error()]       # a zero answer comes with its reason
                rows.append(row)
            out[f"{name}/mode{mode}"] = rows
    return out


def _call(L, entry, desc, lay, n, n_params, n_target, null=(), ws_bytes=0):
    """One call with dummy pointers and workspace_bytes = 0 (or ws_bytes: see _validation) -> (return code, cmcd_last_error)."""
    p = lambda name: None if name in null else PTR
    head = [C.byref(desc), C.byref(lay), p("seeds"), n, p("params"), n_params, p("target_consts"), n_target]
    if entry in FORWARD_LIKE:
        args = head + [p("workspace"), ws_bytes, p("out_loss"), p("out_z"), p("out_stats"), None]
    elif entry == "cmcd_bound_grad":
        args = head + [C.c_float(1.0), p("workspace"), ws_bytes, p("out_loss"), p("out_z"), p("out_stats"), p("grad"), None]
    else:
        args = head + [p("omega"), p("workspace"), 0, p("grad"), None]
    rc = getattr(L, entry)(*args)
    return rc, _lib.last_error()


def _cases():
    """(key, desc, layout, n, n_params, n_target, entry points whose mode this is) on real descriptors and layouts."""
    sn, var = ("cmcd_bound_forward", "cmcd_bound_forward_prepared", "cmcd_bound_grad"), FORWARD_LIKE + VAR_GRADS
    builds = [("gmm_n300_k8", {}, sn), ("funnel_n300_k64", {}, sn), ("many_gmm_n2000_k256_dds", {}, sn),
              ("many_gmm_var_n16000_k256", {}, var), ("many_gmm_var_n16000_k256", {"boundmode": "MCD_CAIS_sn"}, sn),
              ("gmm_n300_k8", {"boundmode": "MCD_CAIS_var_sn"}, var), ("gmm_n300_k8", {"boundmode": "MCD_ULA"}, sn),
              ("gmm_n300_k8", {"boundmode": "MCD_ULA_sn"}, sn), ("funnel_n300_k64", {"boundmode": "MCD_CAIS_UHA_sn"}, sn),
              ("many_gmm_var_n16000_k256", {"boundmode": "MCD_CAIS_UHA_sn"}, sn),
              ("lgcp_n20_k128", {}, sn),
              ("lgcp_n20_k128", {"boundmode": "MCD_CAIS_var_sn"}, FORWARD_LIKE + VAR_GRADS[1:])]   # lgcp: the kept form only
    for cfg, over, entries in builds:
        if cfg.startswith("lgcp"):
            from helpers import lgcp_counts_fixture
            over = dict(over, lgcp_counts=lgcp_counts_fixture())
        b = synthetic.build(cfg, device="cpu", **over)
        plan = mcdbm._plan(b["unflatten"], b["params_fixed"], b["target"], b["eps_schedule"], b["grad_clipping"])
        dim = b["params_fixed"][0]
        targets = {"many_gmm": (1 + 2 * 64, 1 + 2 * 40), "lgcp": (dim * dim + dim + 3,)}.get(b["cfg"]["model"], (0,))
        for n in sorted({b["cfg"]["N"], 20, 300, 2049}):
            for nt in targets:
                key = f"{cfg}/{over.get('boundmode', b['cfg']['boundmode'])}/n{n}/nt{nt}"
                yield key, plan.desc, plan.lay, n, b["params_flat"].numel(), nt, entries


def _needs(L):
    """The 'need N bytes' each entry point reports for workspace_bytes = 0 (None: it refused the call for another reason)."""
    out = {}
    for key, desc, lay, n, n_params, nt, entries in _cases():
        for entry in entries:
            rc, msg = _call(L, entry, desc, lay, n, n_params, nt)
            m = re.search(r"need (\d+) bytes", msg)
            out[f"{key}/{entry}"] = [rc, int(m.group(1)) if m else None, getattr(L, QUERY_OF[entry])(C.byref(desc), n)]
    return out


def _validation(L):
    """Every entry point against: a bad mode, a null pointer, the other gradient's mode, a layout offset outside params_flat,
    bad many_gmm constants, a short workspace — in this order, each call otherwise valid.  cmcd_bound_grad and
    cmcd_bound_var_forward check the workspace before they enter the forward's validation, so an empty workspace hides the steps
    behind that check: they run every step but the last a second time with workspace_bytes = 2^40.  Each of those calls carries
    a defect the forward's validation refuses, so none reaches a launch.  (The two cmcd_bound_var_grad* calls have no check
    of params_flat's length behind their workspace check: with room in the workspace that step would launch, so it is not run.)"""
    sn = synthetic.build("many_gmm_n2000_k256_dds", device="cpu")
    var = synthetic.build("many_gmm_var_n16000_k256", device="cpu")
    out = {}
    for entry in ENTRIES:
        own = var if entry in VAR_GRADS + ("cmcd_bound_var_forward",) else sn
        plan = mcdbm._plan(own["unflatten"], own["params_fixed"], own["target"], own["eps_schedule"], own["grad_clipping"])
        n, n_params, nt = 2000, own["params_flat"].numel(), 1 + 2 * 40
        edit = lambda **kw: _lib.Desc(**{**{k: getattr(plan.desc, k) for k, _ in _lib.Desc._fields_}, **kw})
        steps = [("bad mode", dict(desc=edit(mode=7))),
                 ("null params", dict(null=("params",))),
                 ("null last output", dict(null=("grad", "out_stats"))),
                 ("other gradient's mode", dict(desc=edit(mode=1 - plan.desc.mode))),
                 ("layout outside params_flat", dict(n_params=1)),
                 ("bad many_gmm constants", dict(n_target=4)),
                 ("null many_gmm constants", dict(null=("target_consts",))),
                 ("short workspace", dict())]
        rows = []
        for name, kw in steps:
            rc, msg = _call(L, entry, kw.get("desc", plan.desc), plan.lay, n, kw.get("n_params", n_params),
                            kw.get("n_target", nt), kw.get("null", ()))
            rows.append([name, rc, msg])
        if entry in ("cmcd_bound_grad", "cmcd_bound_var_forward"):
            for name, kw in steps[:-1]:
                rc, msg = _call(L, entry, kw.get("desc", plan.desc), plan.lay, n, kw.get("n_params", n_params),
                                kw.get("n_target", nt), kw.get("null", ()), ws_bytes=1 << 40)
                assert rc != 0, (entry, name)
                rows.append([name + ", room in the workspace", rc, msg])
        out[entry] = rows
    return out


def write_fixture():
    L = _lib.lib()
    with open(FIXTURE, "w") as f:
        json.dump({"library": "f4eb563", "sizes": _sizes(L), "needs": _needs(L), "validation": _validation(L)}, f,
                  indent=0, sort_keys=True)


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE) as f:
        return json.load(f)


def test_size_queries_reproduce_the_stored_answers(hip_lib, golden):
    got = _sizes(hip_lib)
    assert set(got) == set(golden["sizes"]) and len(got) == 5 * len(NETS)
    for key, rows in got.items():
        assert [r[0] for r in rows] == list(NS)
        for row, want in zip(rows, golden["sizes"][key]):
            assert row == want, (key, row, want)
    flat = [r for rows in got.values() for r in rows]
    assert any(r[1] == 0 for r in flat) and any(r[3] == 0 for r in flat) and any(r[1] and r[3] and r[5] for r in flat)


def test_every_entry_point_demands_what_its_size_query_answers(hip_lib, golden):
    """'Query and user agree': with the largest target block (64 mixtures) the demand IS the size query's answer; with 40
    mixtures it is what the library demanded before the plan (the VarGrad calls: still the query's; the others: less)."""
    got = _needs(hip_lib)
    assert set(got) == set(golden["needs"])
    seen = set()
    for key, (rc, need, query) in got.items():
        assert [rc, need, query] == golden["needs"][key], (key, rc, need, query, golden["needs"][key])
        assert rc == -3 and need is not None and query > 0, (key, rc, need)        # CMCD_ERR_WORKSPACE, with its byte count
        entry = key.rsplit("/", 1)[1]
        if "/nt81/" not in key or QUERY_OF[entry] == QUERIES[1]:
            assert need == query, (key, need, query)
        else:
            assert 0 < need < query, (key, need, query)
        seen.add(entry)
    assert seen == set(ENTRIES)


def test_entry_points_refuse_bad_input_in_the_stored_order(hip_lib, golden):
    got = _validation(hip_lib)
    assert set(got) == set(ENTRIES) == set(golden["validation"])
    for entry, rows in got.items():
        assert rows == golden["validation"][entry], (entry, rows, golden["validation"][entry])
        assert all(rc != 0 for _, rc, _ in rows)
        assert rows[0][1:] == [-2, "Mode not implemented."] and any("16-byte aligned" in r[2] for r in rows)
