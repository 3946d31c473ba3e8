"""The workspace plan of the d = 1600 path (csrc/cmcd_lgcp.hip: lgcp_ws, lgcp_uha_ws, lgcp_grad_ws, lgcp_uha_grad_ws;
csrc/cmcd_lgcp_wide.hip: wide_ws), on the CPU: size queries only, nothing is launched.

tests/test_capi_plan.py pins these sizes at emb_dim = 20, reserved = 0 alone.  tests/golden/capi_lgcp_sizes.json holds what the
library answered BEFORE the four host sequences of cmcd_lgcp.hip were put on one set of helpers and one bump allocator (commit
1de700f): cmcd_workspace_bytes, cmcd_grad_workspace_bytes and cmcd_bound_grad_workspace_bytes for target lgcp, dim = 1600 over

    emb_dim   4, 12, 20, 70, 128, 132      IN = 1664 / 1670: the last / first width past the 1st-order no-split-K form,
                                           IN = 3328 / 3332: the same for the 2nd-order form (two rounds of chunks)
    mode      all five
    reserved  0, 1, 2, 3                   the library's choice, 32-row passes pinned, wide path pinned, split-K pinned
    nbridges  1, 128                       with n, both sides of the 2^28-float caps of the kept tables
    n         1, 16, 17, 20, 21, 32, 33, 129, 224, 225, 600      lane counts at 32 / 33 / 129, the wide path at 224 / 225

with the reason of every zero.  It was written from that commit's library with

    CMCD_LIB_PATH=<that commit's libcmcd_hip.so> python -c "import sys; sys.path.insert(0, 'tests'); \
        import test_capi_lgcp_plan as t; t.write_fixture()"

and is not to be regenerated from the library under test."""
import ctypes as C
import json
import os

import pytest

from cmcd_amd import _lib

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "capi_lgcp_sizes.json")
EMBS = (4, 12, 20, 70, 128, 132)
RESERVED = (0, 1, 2, 3)
BRIDGES = (1, 128)
NS = (1, 16, 17, 20, 21, 32, 33, 129, 224, 225, 600)
QUERIES = ("cmcd_workspace_bytes", "cmcd_grad_workspace_bytes", "cmcd_bound_grad_workspace_bytes")
LGCP, DIM = 3, 1600
ULA = 2         # MCD_ULA has no network: the library asks for arch = CMCD_ARCH_DDS as the placeholder


def _sizes(L):
    """-> {"emb/mode/reserved/K": [[answers of the three queries] per n of NS]}; a zero answer is stored as its reason."""
    out = {}
    for emb in EMBS:
        for mode in range(5):
            for res in RESERVED:
                for K in BRIDGES:
                    d = _lib.Desc(dim=DIM, nbridges=K, mode=mode, arch=1 if mode == ULA else 0, emb_dim=emb, target=LGCP,
                                  eps_schedule=2, grad_clipping=1, ngrid=8, reserved=res)
                    rows = []
                    for n in NS:
                        row = []
                        for q in QUERIES:
                            nb = getattr(L, q)(C.byref(d), n)
                            row.append(nb if nb else _lib.last_error())
                        rows.append(row)
                    out[f"emb{emb}/mode{mode}/reserved{res}/K{K}"] = rows
    return out


def _pack(sizes):
    """Rows that repeat an earlier key's are stored as that key (reserved = 1 / 2 / 3 differ from 0 only where they bite)."""
    seen, out = {}, {}
    for key, rows in sizes.items():
        sig = json.dumps(rows)
        out[key] = seen.get(sig, rows)
        seen.setdefault(sig, key)
    return out


def _unpack(stored):
    return {key: stored[rows] if isinstance(rows, str) else rows for key, rows in stored.items()}


def write_fixture():
    with open(FIXTURE, "w") as f:
        json.dump({"library": "1de700f", "ns": list(NS), "sizes": _pack(_sizes(_lib.lib()))}, f, separators=(",", ":"))


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE) as f:
        return json.load(f)


def test_lgcp_size_queries_reproduce_the_stored_answers(hip_lib, golden):
    assert golden["ns"] == list(NS)
    want = _unpack(golden["sizes"])
    got = _sizes(hip_lib)
    assert sorted(got) == sorted(want)
    for key, rows in got.items():
        for n, row, stored in zip(NS, rows, want[key]):
            assert row == stored, (key, n, row, stored)


def test_the_grid_crosses_every_admission_edge(golden):
    """The stored answers themselves: each edge the allocators branch on changes at least one answer."""
    want = _unpack(golden["sizes"])
    at = lambda emb, mode, res, K, n: want[f"emb{emb}/mode{mode}/reserved{res}/K{K}"][NS.index(n)]
    flat = [a for rows in want.values() for row in rows for a in row]
    assert any(isinstance(a, str) for a in flat) and any(isinstance(a, int) and a > 0 for a in flat)
    assert at(20, 0, 0, 1, 20) != at(20, 0, 3, 1, 20)          # IN = 1620: the packed copies and kept tables are there,
    assert at(20, 2, 0, 1, 20) != at(20, 2, 3, 1, 20)          # in MCD_ULA too,
    assert at(70, 0, 0, 1, 20) == at(70, 0, 3, 1, 20)          # at IN = 1670 the split-K form by the library's own choice
    assert at(128, 0, 0, 1, 20) == at(128, 0, 3, 1, 20)
    assert at(128, 4, 0, 1, 20) != at(128, 4, 3, 1, 20)        # 2nd order, IN = 3328: the last width of its no-split-K form
    assert at(132, 4, 0, 1, 20) == at(132, 4, 3, 1, 20)        # IN = 3332: the split-K form by the library's own choice
    # the wide path (the query answers the larger of the two forms: it shows where the 32-row form has no packed copies)
    assert at(132, 0, 0, 1, 224) == at(132, 0, 1, 1, 224) and at(132, 0, 0, 1, 225)[0] > at(132, 0, 1, 1, 225)[0]
    assert at(132, 0, 2, 1, 224)[0] > at(132, 0, 0, 1, 224)[0]
    # the lane count: a second lane's buffers at 33, none at 32
    assert at(20, 0, 0, 1, 33)[0] - at(20, 0, 0, 1, 32)[0] > at(20, 0, 0, 1, 32)[0] - at(20, 0, 0, 1, 21)[0]
    # the 2^28-float cap of the kept tables: the gradient workspace grows by less per particle once they are off
    per_n = lambda emb, mode, K, n0, n1: (at(emb, mode, 0, K, n1)[2] - at(emb, mode, 0, K, n0)[2]) / (n1 - n0)
    assert per_n(20, 0, 128, 225, 600) < per_n(20, 0, 128, 32, 33)
    assert per_n(20, 4, 128, 129, 224) < per_n(20, 4, 128, 32, 33)
