"""cmcd_reverse_uha_workspace_bytes / cmcd_bound_reverse_uha without a GPU: declared, exported, the size query consistent with
the call, and every refusal decided on the host before anything touches the device (all device pointers here are a dummy address
that is never followed).  Mirrors tests/test_capi_segment_uha.py for the reverse-time chain of the mode."""
import ctypes as C
import os
import re

import pytest
import torch

from cmcd_amd import _lib, build, synthetic
from cmcd_amd import mcdboundingmachine as mcdbm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = C.c_void_p(16)        # "some non-null device pointer": a refused call never reads it
NAMES = ("cmcd_reverse_uha_workspace_bytes", "cmcd_bound_reverse_uha")
MODE = "MCD_CAIS_UHA_sn"


def plan_of(name="gmm_n300_k8", **over):
    b = synthetic.build(name, device="cpu", **dict(dict(boundmode=MODE), **over))
    return b, mcdbm._plan(b["unflatten"], b["params_fixed"], b["target"], b["eps_schedule"], b["grad_clipping"])


def call(lib, b, plan, seeds=P, x=P, n=32, ws=P, ws_bytes=1 << 40, w=P, z0=P, rho0=P, stats=P, desc=None, params=P, consts=None,
         n_consts=0):
    return lib.cmcd_bound_reverse_uha(C.byref(desc if desc is not None else plan.desc), C.byref(plan.lay), seeds, x, n, params,
                                      b["params_flat"].numel(), consts, n_consts, ws, ws_bytes, w, z0, rho0, stats, None)


def lgcp_desc(plan):
    return _lib.Desc(dim=1600, nbridges=2, mode=plan.desc.mode, arch=0, emb_dim=20, target=3, eps_schedule=0, grad_clipping=0, ngrid=2,
                     reserved=0)


def test_header_declares_and_library_exports_the_entry_points(hip_lib):
    src = open(os.path.join(ROOT, "include", "cmcd_hip.h")).read()
    assert "rho_i = m_b + sigma_i xi_r" in src                    # the arithmetic is written out in the header ...
    assert "rho_K = normal(R, (dim,))" in src and "gen_0 = second(split(G'))" in src      # ... and so is the key chain
    assert "no reverse-time chain" not in src
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(cmcd_[a-z_0-9]+)\s*\(", src))
    for name in NAMES:
        assert name in declared, f"{name} is not declared in include/cmcd_hip.h"
        assert hasattr(hip_lib, name), f"{name} is not exported"
    assert hip_lib.cmcd_version() == 3      # additive: the ABI version does not move
    assert "cmcd_reverse_uha.hip" in build.SOURCES and build.EXTRA_FLAGS["cmcd_reverse_uha.hip"] == ["-fno-slp-vectorize"]


# gmm geffner 24 / 44 (2 / 4 tiles) and dds; funnel geffner 68 / 120 (5 / 9 tiles); many_gmm geffner 134 (9 tiles)
@pytest.mark.parametrize("name,over,n", [("gmm_n300_k8", {}, 1), ("gmm_n300_k8", dict(emb_dim=40), 300), ("gmm_n300_k8", dict(nn_arch="dds"), 33),
                                          ("funnel_n300_k64", {}, 17), ("funnel_n300_k64", dict(emb_dim=100), 300),
                                          ("many_gmm_var_n16000_k256", {}, 2000)])
def test_size_query_is_the_forward_layout_and_what_the_call_demands(hip_lib, name, over, n):
    b, plan = plan_of(name, **over)
    need = hip_lib.cmcd_reverse_uha_workspace_bytes(C.byref(plan.desc), n)
    assert need > 0 and need % 4 == 0 and need == hip_lib.cmcd_workspace_bytes(C.byref(plan.desc), n)
    consts = b["target"].consts_on("cpu")
    kw = {} if consts is None else dict(consts=P, n_consts=consts.numel())
    short = need - 1 if consts is None else need // 2
    for ws, nbytes in ((P, short), (C.c_void_p(24), need)):                     # short, not 16-byte aligned
        assert call(hip_lib, b, plan, n=n, ws=ws, ws_bytes=nbytes, **kw) == -3
        if consts is None:
            assert _lib.last_error() == f"workspace too small or not 16-byte aligned (need {need} bytes)"


def test_size_query_answers_zero_to_what_the_call_refuses(hip_lib):
    _, plan = plan_of()
    assert hip_lib.cmcd_reverse_uha_workspace_bytes(C.byref(plan.desc), 0) == 0
    assert hip_lib.cmcd_reverse_uha_workspace_bytes(None, 32) == 0
    for mode in ("MCD_CAIS_sn", "MCD_CAIS_var_sn", "MCD_ULA", "MCD_ULA_sn"):      # every overdamped mode
        _, p = plan_of(boundmode=mode)
        assert hip_lib.cmcd_reverse_uha_workspace_bytes(C.byref(p.desc), 32) == 0
        assert "the overdamped modes have cmcd_bound_reverse" in _lib.last_error()
    _, p = plan_of(emb_dim=198)                                                    # width 202
    assert hip_lib.cmcd_reverse_uha_workspace_bytes(C.byref(p.desc), 32) == 0
    assert "kernel instance" in _lib.last_error() and "width=208" in _lib.last_error()
    assert hip_lib.cmcd_reverse_uha_workspace_bytes(C.byref(lgcp_desc(plan)), 32) == 0
    assert "the reverse chain has no lgcp kernel" in _lib.last_error()
    # ... and the overdamped call keeps refusing this mode
    assert hip_lib.cmcd_reverse_workspace_bytes(C.byref(plan.desc), 32) == 0 and "overdamped modes only" in _lib.last_error()


def test_refusals_are_decided_before_any_gpu_work(hip_lib):
    b, plan = plan_of()
    cases = [
        (dict(seeds=None), -1, "null pointer"),
        (dict(x=None), -1, "null pointer"),
        (dict(w=None), -1, "null pointer"),
        (dict(z0=None), -1, "null pointer"),
        (dict(rho0=None), -1, "null pointer"),
        (dict(stats=None), -1, "null pointer"),
        (dict(ws=None), -1, "null pointer"),
        (dict(params=None), -1, "null pointer"),
        (dict(n=0), -1, "n out of range"),
        (dict(n=-5), -1, "n out of range"),
        (dict(ws_bytes=64), -3, "workspace too small"),
        (dict(ws=C.c_void_p(24)), -3, "16-byte aligned"),
    ]
    for kw, status, text in cases:
        rc = call(hip_lib, b, plan, **kw)
        assert rc == status, (kw, rc, _lib.last_error())
        assert text in _lib.last_error(), (kw, _lib.last_error())
    # no kernel: the overdamped modes, a width without an instance, lgcp
    for mode in ("MCD_CAIS_sn", "MCD_CAIS_var_sn", "MCD_ULA", "MCD_ULA_sn"):
        bo, po = plan_of(boundmode=mode)
        assert call(hip_lib, bo, po) == -2 and "cmcd_bound_reverse" in _lib.last_error()
    bw, pw = plan_of(emb_dim=198)
    assert call(hip_lib, bw, pw) == -2 and "kernel instance" in _lib.last_error() and "width=208" in _lib.last_error()
    assert call(hip_lib, b, plan, desc=lgcp_desc(plan)) == -2 and "lgcp" in _lib.last_error()
    with pytest.raises(NotImplementedError):
        _lib.check(call(hip_lib, bo, po))
    with pytest.raises(ValueError):
        _lib.check(call(hip_lib, b, plan, x=None))
    # a layout that points outside params_flat, many_gmm without its constants
    short = lambda: hip_lib.cmcd_bound_reverse_uha(C.byref(plan.desc), C.byref(plan.lay), P, P, 32, P, 10, None, 0, P, 1 << 40, P, P, P,
                                                   P, None)
    assert short() == -1 and "layout offset" in _lib.last_error()
    bm, pm = plan_of("many_gmm_n2000_k256_dds", nbridges=8)
    assert call(hip_lib, bm, pm) == -1 and "many_gmm needs target_consts" in _lib.last_error()


def test_python_entry_points_refuse_host_tensors(hip_lib):
    from cmcd_amd import reverse_uha
    assert reverse_uha.__all__ == ["bound_reverse", "compute_reverse_bound"]
    b, _ = plan_of()
    args = (b["params_flat"], b["unflatten"], b["params_fixed"], b["target"])
    seeds = torch.arange(1, 33, dtype=torch.int32)
    for fn in (reverse_uha.bound_reverse, reverse_uha.compute_reverse_bound):
        with pytest.raises(RuntimeError, match="runs on a ROCm device only"):
            fn(seeds, torch.zeros(32, 2), *args)
