"""cmcd_segment_workspace_bytes / cmcd_bound_segment without a GPU: declared, exported, the size query consistent with the call,
and every refusal decided on the host before anything touches the device (all device pointers here are a dummy address that
is never followed)."""
import ctypes as C
import os
import re

import pytest
import torch

from cmcd_amd import _lib, synthetic
from cmcd_amd import mcdboundingmachine as mcdbm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = C.c_void_p(16)        # "some non-null device pointer": a refused call never reads it
NAMES = ("cmcd_segment_workspace_bytes", "cmcd_bound_segment")


def plan_of(name="gmm_n300_k8", **over):
    b = synthetic.build(name, device="cpu", **over)
    return b, mcdbm._plan(b["unflatten"], b["params_fixed"], b["target"], b["eps_schedule"], b["grad_clipping"])


def call(lib, b, plan, k0=0, k1=2, seeds=P, n=32, ws=P, ws_bytes=1 << 40, z=P, wpath=P, key=P, lg=P, stats=P, desc=None, params=P,
         consts=None, n_consts=0):
    return lib.cmcd_bound_segment(C.byref(desc if desc is not None else plan.desc), C.byref(plan.lay), k0, k1, seeds, n, params,
                                  b["params_flat"].numel(), consts, n_consts, ws, ws_bytes, z, wpath, key, lg, stats, None)


def test_header_declares_and_library_exports_the_entry_points(hip_lib):
    src = open(os.path.join(ROOT, "include", "cmcd_hip.h")).read()
    assert "log gamma_k = beta_{k-1} log p + (1 - beta_{k-1}) log q" in src       # the arithmetic is written out in the header
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(cmcd_[a-z_0-9]+)\s*\(", src))
    for name in NAMES:
        assert name in declared, f"{name} is not declared in include/cmcd_hip.h"
        assert hasattr(hip_lib, name), f"{name} is not exported"
    assert hip_lib.cmcd_version() == 3      # additive: the ABI version does not move


@pytest.mark.parametrize("name,over,n", [("gmm_n300_k8", {}, 1), ("gmm_n300_k8", dict(boundmode="MCD_ULA"), 300),
                                          ("funnel_n300_k64", dict(nn_arch="dds"), 17), ("many_gmm_var_n16000_k256", {}, 2000)])
def test_size_query_is_the_forward_layout_and_what_the_call_demands(hip_lib, name, over, n):
    b, plan = plan_of(name, **over)
    need = hip_lib.cmcd_segment_workspace_bytes(C.byref(plan.desc), n)
    assert need > 0 and need % 4 == 0 and need == hip_lib.cmcd_workspace_bytes(C.byref(plan.desc), n)
    consts = b["target"].consts_on("cpu")
    kw = {} if consts is None else dict(consts=P, n_consts=consts.numel())
    # (with target constants the call lays out this call's block and the query the largest one: only then may need - 1 suffice)
    short = need - 1 if consts is None else need // 2
    for ws, nbytes in ((P, short), (C.c_void_p(24), need)):                     # short, not 16-byte aligned
        assert call(hip_lib, b, plan, n=n, ws=ws, ws_bytes=nbytes, **kw) == -3
        if consts is None:
            assert _lib.last_error() == f"workspace too small or not 16-byte aligned (need {need} bytes)"


def test_size_query_answers_zero_to_what_the_call_refuses(hip_lib):
    _, plan = plan_of()
    assert hip_lib.cmcd_segment_workspace_bytes(C.byref(plan.desc), 0) == 0
    assert hip_lib.cmcd_segment_workspace_bytes(None, 32) == 0
    for over in (dict(boundmode="MCD_CAIS_UHA_sn"), dict(emb_dim=200)):
        _, p = plan_of(**over)
        assert hip_lib.cmcd_segment_workspace_bytes(C.byref(p.desc), 32) == 0
    lgcp = _lib.Desc(dim=1600, nbridges=2, mode=0, arch=0, emb_dim=20, target=3, eps_schedule=0, grad_clipping=0, ngrid=2, reserved=0)
    assert hip_lib.cmcd_segment_workspace_bytes(C.byref(lgcp), 32) == 0 and "lgcp" in _lib.last_error()


def test_refusals_are_decided_before_any_gpu_work(hip_lib):
    b, plan = plan_of()          # K = 8
    cases = [
        (dict(k0=-1), -1, "0 <= k0 < k1 <= nbridges"),
        (dict(k0=2, k1=2), -1, "0 <= k0 < k1 <= nbridges"),
        (dict(k0=3, k1=2), -1, "0 <= k0 < k1 <= nbridges"),
        (dict(k1=9), -1, "0 <= k0 < k1 <= nbridges"),
        (dict(k0=8, k1=9), -1, "0 <= k0 < k1 <= nbridges"),
        (dict(seeds=None), -1, "needs seeds"),
        (dict(z=None, k0=1), -1, "null pointer"),
        (dict(wpath=None), -1, "null pointer"),
        (dict(key=None), -1, "null pointer"),
        (dict(lg=None), -1, "null pointer"),
        (dict(stats=None), -1, "null pointer"),
        (dict(ws=None), -1, "null pointer"),
        (dict(params=None), -1, "null pointer"),
        (dict(n=0), -1, "n out of range"),
        (dict(ws_bytes=64), -3, "workspace too small"),
    ]
    for kw, status, text in cases:
        rc = call(hip_lib, b, plan, **kw)
        assert rc == status, (kw, rc, _lib.last_error())
        assert text in _lib.last_error(), (kw, _lib.last_error())
    # a null seeds pointer is fine past bridge 0: the call gets as far as the workspace check
    assert call(hip_lib, b, plan, k0=1, k1=2, seeds=None, ws_bytes=64) == -3
    # no kernel: 2nd-order CMCD, lgcp, a width without an instance
    bu, pu = plan_of(boundmode="MCD_CAIS_UHA_sn")
    assert call(hip_lib, bu, pu) == -2 and "overdamped modes only" in _lib.last_error()
    bw, pw = plan_of(emb_dim=200)
    assert call(hip_lib, bw, pw) == -2 and "no kernel instance" in _lib.last_error()
    lgcp = _lib.Desc(dim=1600, nbridges=2, mode=0, arch=0, emb_dim=20, target=3, eps_schedule=0, grad_clipping=0, ngrid=2, reserved=0)
    assert call(hip_lib, b, plan, desc=lgcp) == -2 and "lgcp" in _lib.last_error()
    with pytest.raises(NotImplementedError):
        _lib.check(call(hip_lib, bu, pu))
    with pytest.raises(ValueError):
        _lib.check(call(hip_lib, b, plan, k1=9))
    # a layout that points outside params_flat, many_gmm without its constants
    short = lambda: hip_lib.cmcd_bound_segment(C.byref(plan.desc), C.byref(plan.lay), 0, 2, P, 32, P, 10, None, 0, P, 1 << 40, P, P, P,
                                               P, P, None)
    assert short() == -1 and "layout offset" in _lib.last_error()
    bm, pm = plan_of("many_gmm_n2000_k256_dds", nbridges=8)
    assert call(hip_lib, bm, pm) == -1 and "many_gmm needs target_consts" in _lib.last_error()


def test_python_entry_points_refuse_cpu_tensors(hip_lib):
    from cmcd_amd import smc
    b, _ = plan_of()
    args = (b["params_flat"], b["unflatten"], b["params_fixed"], b["target"])
    seeds = torch.arange(1, 33, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="runs on a ROCm device only"):
        smc.segment(seeds, 0, 2, *args)
    state = {"z": torch.zeros(32, 2), "wpath": torch.zeros(32), "key": torch.zeros(32, 2, dtype=torch.int32)}
    with pytest.raises(RuntimeError, match="runs on a ROCm device only"):
        smc.segment(state, 2, 4, *args)
    with pytest.raises(RuntimeError, match="runs on a ROCm device only"):
        smc.smc_bound(seeds, *args, groups=2)
    with pytest.raises(ValueError, match="cuts"):
        smc.smc_bound(seeds, *args, cuts=[3, 3])
    assert smc.default_cuts(8) == [1, 2, 3, 4, 5, 6, 7] and smc.default_cuts(256) == list(range(32, 256, 32)) and smc.default_cuts(1) == []
