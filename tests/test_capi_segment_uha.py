"""cmcd_segment_uha_workspace_bytes / cmcd_bound_segment_uha without a GPU: declared, exported, the size query consistent with
the call, and every refusal decided on the host before anything touches the device (all device pointers here are a dummy address
that is never followed).  Mirrors tests/test_capi_segment.py for the state with momentum."""
import ctypes as C
import os
import re

import pytest
import torch

from cmcd_amd import _lib, build, synthetic
from cmcd_amd import mcdboundingmachine as mcdbm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = C.c_void_p(16)        # "some non-null device pointer": a refused call never reads it
NAMES = ("cmcd_segment_uha_workspace_bytes", "cmcd_bound_segment_uha")
MODE = "MCD_CAIS_UHA_sn"


def plan_of(name="gmm_n300_k8", **over):
    b = synthetic.build(name, device="cpu", **dict(dict(boundmode=MODE), **over))
    return b, mcdbm._plan(b["unflatten"], b["params_fixed"], b["target"], b["eps_schedule"], b["grad_clipping"])


def call(lib, b, plan, k0=0, k1=2, seeds=P, n=32, ws=P, ws_bytes=1 << 40, z=P, rho=P, wpath=P, key=P, lg=P, stats=P, desc=None,
         params=P, consts=None, n_consts=0):
    return lib.cmcd_bound_segment_uha(C.byref(desc if desc is not None else plan.desc), C.byref(plan.lay), k0, k1, seeds, n, params,
                                      b["params_flat"].numel(), consts, n_consts, ws, ws_bytes, z, rho, wpath, key, lg, stats, None)


def test_header_declares_and_library_exports_the_entry_points(hip_lib):
    src = open(os.path.join(ROOT, "include", "cmcd_hip.h")).read()
    assert "lg = log gamma_k1(z) + log N(rho; 0, I)" in src       # the arithmetic is written out in the header
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(cmcd_[a-z_0-9]+)\s*\(", src))
    for name in NAMES:
        assert name in declared, f"{name} is not declared in include/cmcd_hip.h"
        assert hasattr(hip_lib, name), f"{name} is not exported"
    assert hip_lib.cmcd_version() == 3      # additive: the ABI version does not move
    assert "cmcd_segment_uha.hip" in build.SOURCES and build.EXTRA_FLAGS["cmcd_segment_uha.hip"] == ["-fno-slp-vectorize"]


# gmm geffner 24 / 44 (2 / 4 tiles) and dds; funnel geffner 68 / 120 (5 / 9 tiles); many_gmm geffner 134 (9 tiles)
@pytest.mark.parametrize("name,over,n", [("gmm_n300_k8", {}, 1), ("gmm_n300_k8", dict(emb_dim=40), 300), ("gmm_n300_k8", dict(nn_arch="dds"), 33),
                                          ("funnel_n300_k64", {}, 17), ("funnel_n300_k64", dict(emb_dim=100), 300),
                                          ("many_gmm_var_n16000_k256", {}, 2000)])
def test_size_query_is_the_forward_layout_and_what_the_call_demands(hip_lib, name, over, n):
    b, plan = plan_of(name, **over)
    need = hip_lib.cmcd_segment_uha_workspace_bytes(C.byref(plan.desc), n)
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
    assert hip_lib.cmcd_segment_uha_workspace_bytes(C.byref(plan.desc), 0) == 0
    assert hip_lib.cmcd_segment_uha_workspace_bytes(None, 32) == 0
    for mode in ("MCD_CAIS_sn", "MCD_CAIS_var_sn", "MCD_ULA", "MCD_ULA_sn"):      # every overdamped mode
        _, p = plan_of(boundmode=mode)
        assert hip_lib.cmcd_segment_uha_workspace_bytes(C.byref(p.desc), 32) == 0 and "cmcd_bound_segment" in _lib.last_error()
    _, p = plan_of(emb_dim=198)                                                    # width 202
    assert hip_lib.cmcd_segment_uha_workspace_bytes(C.byref(p.desc), 32) == 0
    lgcp = _lib.Desc(dim=1600, nbridges=2, mode=plan.desc.mode, arch=0, emb_dim=20, target=3, eps_schedule=0, grad_clipping=0, ngrid=2,
                     reserved=0)
    assert hip_lib.cmcd_segment_uha_workspace_bytes(C.byref(lgcp), 32) == 0 and "lgcp" in _lib.last_error()
    # ... and the overdamped call keeps refusing this mode
    assert hip_lib.cmcd_segment_workspace_bytes(C.byref(plan.desc), 32) == 0 and "overdamped modes only" in _lib.last_error()


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
        (dict(rho=None), -1, "null pointer"),
        (dict(rho=None, k0=1), -1, "null pointer"),
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
    # no kernel: the overdamped modes, lgcp, a width without an instance
    bo, po = plan_of(boundmode="MCD_CAIS_sn")
    assert call(hip_lib, bo, po) == -2 and "cmcd_bound_segment" in _lib.last_error()
    bw, pw = plan_of(emb_dim=198)
    assert call(hip_lib, bw, pw) == -2
    lgcp = _lib.Desc(dim=1600, nbridges=2, mode=plan.desc.mode, arch=0, emb_dim=20, target=3, eps_schedule=0, grad_clipping=0, ngrid=2,
                     reserved=0)
    assert call(hip_lib, b, plan, desc=lgcp) == -2 and "lgcp" in _lib.last_error()
    with pytest.raises(NotImplementedError):
        _lib.check(call(hip_lib, bo, po))
    with pytest.raises(ValueError):
        _lib.check(call(hip_lib, b, plan, k1=9))
    # a layout that points outside params_flat, many_gmm without its constants
    short = lambda: hip_lib.cmcd_bound_segment_uha(C.byref(plan.desc), C.byref(plan.lay), 0, 2, P, 32, P, 10, None, 0, P, 1 << 40, P, P,
                                                   P, P, P, P, None)
    assert short() == -1 and "layout offset" in _lib.last_error()
    bm, pm = plan_of("many_gmm_n2000_k256_dds", nbridges=8)
    assert call(hip_lib, bm, pm) == -1 and "many_gmm needs target_consts" in _lib.last_error()


def test_python_entry_points_refuse_cpu_tensors_and_states_without_momentum(hip_lib):
    from cmcd_amd import smc, smc_uha
    assert smc_uha.STATE_FIELDS == ("z", "rho", "wpath", "lg", "key") and smc_uha.losses_of is smc.losses_of
    b, _ = plan_of()
    args = (b["params_flat"], b["unflatten"], b["params_fixed"], b["target"])
    seeds = torch.arange(1, 33, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="runs on a ROCm device only"):
        smc_uha.segment(seeds, 0, 2, *args)
    state = {"z": torch.zeros(32, 2), "rho": torch.zeros(32, 2), "wpath": torch.zeros(32), "key": torch.zeros(32, 2, dtype=torch.int32)}
    with pytest.raises(RuntimeError, match="runs on a ROCm device only"):
        smc_uha.segment(state, 2, 4, *args)
    with pytest.raises(TypeError, match="rho"):
        smc_uha.segment({k: v for k, v in state.items() if k != "rho"}, 2, 4, *args)
    with pytest.raises(RuntimeError, match="runs on a ROCm device only"):
        smc_uha.smc_bound(seeds, *args, groups=2)
    with pytest.raises(ValueError, match="cuts"):
        smc_uha.smc_bound(seeds, *args, cuts=[3, 3])
    bo = synthetic.build("gmm_n300_k8", device="cpu")                            # an overdamped mode: cmcd_amd.smc's
    with pytest.raises(NotImplementedError, match="cmcd_amd.smc"):
        smc_uha.segment(seeds, 0, 2, bo["params_flat"], bo["unflatten"], bo["params_fixed"], bo["target"])
    assert smc_uha.default_cuts(8) == [1, 2, 3, 4, 5, 6, 7]
