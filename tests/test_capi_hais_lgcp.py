"""cmcd_hais_lgcp_workspace_bytes / cmcd_hais_lgcp_bound_grad without a GPU: declared, exported, the size query consistent with
the call, and every refusal decided on the host before anything touches the device (all device pointers here are a dummy
address that is never followed)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import hais_restatement as hr
from cmcd_amd import _lib, hais, hais_lgcp, model_handler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = C.c_void_p(16)        # "some non-null device pointer": a refused call never reads it
NAMES = ("cmcd_hais_lgcp_workspace_bytes", "cmcd_hais_lgcp_bound_grad")
D = 1600
N_TARGET = D * D + D + 3


def case(K=8, L=2):
    flat, un, fixed = hr.make_params(D, K, L, 0.05)
    return flat, un, hais._layout(un)


def call(lib, lay, n_params, dim=D, K=8, L=2, seeds=P, n=37, params=P, consts=P, n_consts=N_TARGET, ws=P, ws_bytes=1 << 40,
         loss=P, z=P, stats=P, grad=P, layout=True):
    return lib.cmcd_hais_lgcp_bound_grad(dim, K, L, C.byref(lay) if layout else None, seeds, n, params, n_params, consts, n_consts,
                                         1.0 / n if n else 1.0, ws, ws_bytes, loss, z, stats, grad, None)


def test_header_declares_and_both_libraries_export_the_entry_points(hip_lib):
    src = open(os.path.join(ROOT, "include", "cmcd_hip.h")).read()
    assert "2 (nbridges L + 1) + 2 nbridges + 1 rows" in src         # the kept rows are stated in the header
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(cmcd_[a-z_0-9]+)\s*\(", src))
    for name in NAMES:
        assert name in declared, f"{name} is not declared in include/cmcd_hip.h"
        assert hasattr(hip_lib, name), f"{name} is not exported"
    assert hip_lib.cmcd_version() == 3      # additive: the ABI version does not move
    from cmcd_amd import build
    assert "cmcd_hais_lgcp.hip" in build.SOURCES


def test_size_query_grows_with_n_K_L_and_the_gradient(hip_lib):
    q = hip_lib.cmcd_hais_lgcp_workspace_bytes
    fwd, both = q(D, 8, 2, 37, 0), q(D, 8, 2, 37, 1)
    assert fwd > 0 and fwd % 16 == 0 and both > fwd and both % 16 == 0
    rows = lambda K, L: 2 * (K * L + 1) + 2 * K + 1                    # the kept rows the header names
    assert both - fwd >= 4 * rows(8, 2) * 37 * D
    assert fwd >= 4 * 5 * 37 * D                                       # z twice, r, rho, w
    assert q(D, 8, 2, 38, 0) > fwd and q(D, 9, 2, 37, 0) > fwd
    assert q(D, 8, 2, 38, 1) - both >= 4 * rows(8, 2) * D
    assert q(D, 9, 2, 37, 1) - both >= 4 * (rows(9, 2) - rows(8, 2)) * 37 * D
    assert q(D, 8, 3, 37, 1) - both >= 4 * (rows(8, 3) - rows(8, 2)) * 37 * D
    for dim in (2, 10, 1599, 1601, 1616, 3200):
        assert q(dim, 8, 1, 37, 0) == 0 and "no Hamiltonian AIS lgcp kernel for this dim" in _lib.last_error()
    for K, L, n in ((0, 1, 37), (8, 0, 37), (8, 1, 0), (-1, 1, 37)):
        assert q(D, K, L, n, 0) == 0 and _lib.last_error()
    assert q(D, 4097, 1, 37, 0) == 0 and "nbridges above 4096" in _lib.last_error()
    assert q(D, 4096, 4097, 37, 0) == 0 and "2^24" in _lib.last_error()
    assert q(D, 8, 1, (1 << 20) + 1, 0) == 0 and "n above 2^20" in _lib.last_error()


def test_size_query_is_what_the_call_demands(hip_lib):
    flat, un, lay = case()
    for with_grad in (0, 1):
        need = hip_lib.cmcd_hais_lgcp_workspace_bytes(D, 8, 2, 37, with_grad)
        g = P if with_grad else None
        assert call(hip_lib, lay, flat.numel(), ws_bytes=need - 16, grad=g) == -3 and "workspace too small" in _lib.last_error()
        assert call(hip_lib, lay, flat.numel(), ws=C.c_void_p(24), ws_bytes=need, grad=g) == -3     # not 16-byte aligned


def test_refusals_are_decided_before_any_gpu_work(hip_lib):
    flat, un, lay = case()
    n_params = flat.numel()
    cases = [
        (dict(seeds=None), -1, "null pointer"),
        (dict(params=None), -1, "null pointer"),
        (dict(consts=None), -1, "null pointer"),
        (dict(ws=None), -1, "null pointer"),
        (dict(loss=None), -1, "null pointer"),
        (dict(z=None), -1, "null pointer"),
        (dict(stats=None), -1, "null pointer"),
        (dict(layout=False), -1, "null pointer"),
        (dict(K=0), -1, "nbridges and lfsteps must be >= 1"),
        (dict(L=0), -1, "nbridges and lfsteps must be >= 1"),
        (dict(n=0), -1, "n or dim out of range"),
        (dict(dim=0), -1, "n or dim out of range"),
        (dict(dim=2), -2, "no Hamiltonian AIS lgcp kernel for this dim"),
        (dict(dim=1616), -2, "no Hamiltonian AIS lgcp kernel for this dim"),
        (dict(K=4097), -2, "nbridges above 4096"),
        (dict(n=(1 << 20) + 1), -2, "n above 2^20"),
        (dict(n_consts=N_TARGET - 1), -1, "lgcp needs target_consts"),
        (dict(n_consts=N_TARGET + 1), -1, "lgcp needs target_consts"),
        (dict(consts=C.c_void_p(20)), -1, "target_consts must be 16-byte aligned"),
        (dict(ws_bytes=64), -3, "workspace too small"),
    ]
    for kw, status, text in cases:
        rc = call(hip_lib, lay, n_params, **kw)
        assert rc == status, (kw, rc, _lib.last_error())
        assert text in _lib.last_error(), (kw, _lib.last_error())
    # every offset of the layout must lie inside params_flat
    for field in _lib.HAIS_LAYOUT_FIELDS[:-1]:
        for bad in (-1, n_params):
            broken = _lib.HaisLayout(**{f: getattr(lay, f) for f in _lib.HAIS_LAYOUT_FIELDS})
            setattr(broken, field, bad)
            assert call(hip_lib, broken, n_params) == -1 and "layout offset" in _lib.last_error(), (field, bad)
    assert call(hip_lib, lay, 10) == -1 and "layout offset" in _lib.last_error()
    for ngrid in (-1, 1025):
        broken = _lib.HaisLayout(**{f: getattr(lay, f) for f in _lib.HAIS_LAYOUT_FIELDS})
        broken.ngrid = ngrid
        assert call(hip_lib, broken, n_params) == -1 and "ngrid" in _lib.last_error()
    with pytest.raises(NotImplementedError):
        _lib.check(call(hip_lib, lay, n_params, dim=2))
    with pytest.raises(ValueError):
        _lib.check(call(hip_lib, lay, n_params, L=0))


def test_python_entry_points_pick_their_target_before_they_need_a_device(hip_lib):
    from cmcd_amd.lgcp import load_model_lgcp
    from helpers import lgcp_counts_fixture
    assert hais_lgcp.initialize is __import__("cmcd_amd.boundingmachine", fromlist=["initialize"]).initialize
    seeds = torch.arange(1, 9, dtype=torch.int32)
    flat2, un2, fixed2 = hr.make_params(2, 8, 1, 0.05)
    gmm = model_handler.load_model("gmm")[0]
    for fn in (hais_lgcp.compute_bound, hais_lgcp.grad_and_loss, hais_lgcp.bound_forward):
        with pytest.raises(NotImplementedError, match="cmcd_amd.hais"):
            fn(seeds, flat2, un2, fixed2, gmm)
        with pytest.raises(TypeError, match="log_prob must be a cmcd_amd.model_handler.Target"):
            fn(seeds, flat2, un2, fixed2, lambda z: z.sum())
    lgcp = load_model_lgcp("lgcp", None, flat_bin_counts=lgcp_counts_fixture())[0]
    assert lgcp.consts_on("cpu").numel() == N_TARGET
    flat, un, fixed = hr.make_params(D, 2, 1, 0.02)
    assert fixed == (D, 2, 1)
    for fn in (hais_lgcp.compute_bound, hais_lgcp.grad_and_loss):
        with pytest.raises(RuntimeError, match="runs on a ROCm device only"):
            fn(seeds, flat, un, fixed, lgcp)
        with pytest.raises(ValueError, match="lfsteps"):
            fn(seeds, flat, un, (D, 2, 0), lgcp)
        with pytest.raises(ValueError, match="target dim 1600 != params_fixed dim 2"):
            fn(seeds, flat, un, (2, 2, 1), lgcp)
        with pytest.raises(RuntimeError, match="runs on a ROCm device only"):      # nbridges = 0: the mean-field bound's own checks
            fn(seeds, flat, un, (D, 0, 1), lgcp)
    # the existing entry points keep refusing lgcp, and say where it went
    assert hip_lib.cmcd_hais_workspace_bytes(3, D, 2, 1, 8, 0) == 0
    assert "lgcp" in _lib.last_error() and "cmcd_hais_lgcp_bound_grad" in _lib.last_error()
