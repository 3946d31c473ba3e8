"""cmcd_hais_workspace_bytes / cmcd_hais_bound_grad without a GPU: declared, exported, the size query consistent with the call,
and every refusal decided on the host before anything touches the device (all device pointers here are a dummy address that
is never followed)."""
import ctypes as C
import os
import re

import pytest
import torch

import hais_restatement as hr
from cmcd_amd import _lib, hais, model_handler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = C.c_void_p(16)        # "some non-null device pointer": a refused call never reads it
NAMES = ("cmcd_hais_workspace_bytes", "cmcd_hais_bound_grad")
GMM, FUNNEL, MANY_GMM, LGCP = 0, 1, 2, 3


def case(dim=2, K=8, L=2):
    flat, un, fixed = hr.make_params(dim, K, L, 0.05)
    return flat, un, hais._layout(un)


def call(lib, lay, n_params, target=GMM, dim=2, K=8, L=2, seeds=P, n=37, params=P, consts=None, n_consts=0, ws=P, ws_bytes=1 << 40,
         loss=P, z=P, stats=P, grad=P, layout=True):
    return lib.cmcd_hais_bound_grad(target, dim, K, L, C.byref(lay) if layout else None, seeds, n, params, n_params, consts, n_consts,
                                    1.0 / n if n else 1.0, ws, ws_bytes, loss, z, stats, grad, None)


def test_header_declares_and_library_exports_the_entry_points(hip_lib):
    src = open(os.path.join(ROOT, "include", "cmcd_hip.h")).read()
    assert "rho = eta rho_prev + sqrt(1 - eta^2) s xi" in src        # the arithmetic is written out in the header
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(cmcd_[a-z_0-9]+)\s*\(", src))
    for name in NAMES:
        assert name in declared, f"{name} is not declared in include/cmcd_hip.h"
        assert hasattr(hip_lib, name), f"{name} is not exported"
    assert hip_lib.cmcd_version() == 3      # additive: the ABI version does not move
    assert C.sizeof(_lib.HaisLayout) == 8 * 9 == 8 * len(_lib.HAIS_LAYOUT_FIELDS)


def test_size_query_answers_for_the_three_targets_and_grows_with_the_gradient(hip_lib):
    q = hip_lib.cmcd_hais_workspace_bytes
    for target, dim in ((GMM, 2), (MANY_GMM, 2), (FUNNEL, 10)):
        fwd, both = q(target, dim, 8, 2, 37, 0), q(target, dim, 8, 2, 37, 1)
        assert fwd > 0 and fwd % 16 == 0 and both > fwd and both % 16 == 0
        # the kept rows: K L + 1 positions, K refreshed momenta, K + 1 momenta between the bridges
        assert both - fwd >= 4 * (8 * 2 + 1 + 2 * 8 + 1) * 37 * dim
        assert q(target, dim, 8, 2, 1040, 0) > fwd and q(target, dim, 8, 3, 37, 1) > both
    assert q(LGCP, 1600, 8, 1, 37, 0) == 0 and "lgcp" in _lib.last_error()
    assert q(FUNNEL, 2, 8, 1, 37, 0) == 0 and "no Hamiltonian AIS kernel instance" in _lib.last_error()
    assert q(GMM, 3, 8, 1, 37, 1) == 0
    for K, L, n in ((0, 1, 37), (8, 0, 37), (8, 1, 0), (-1, 1, 37)):
        assert q(GMM, 2, K, L, n, 0) == 0


def test_size_query_is_what_the_call_demands(hip_lib):
    flat, un, lay = case()
    for with_grad in (0, 1):
        need = hip_lib.cmcd_hais_workspace_bytes(GMM, 2, 8, 2, 37, with_grad)
        g = P if with_grad else None
        assert call(hip_lib, lay, flat.numel(), ws_bytes=need - 1, grad=g) == -3 and "workspace too small" in _lib.last_error()
        assert call(hip_lib, lay, flat.numel(), ws=C.c_void_p(24), ws_bytes=need, grad=g) == -3     # not 16-byte aligned


def test_refusals_are_decided_before_any_gpu_work(hip_lib):
    flat, un, lay = case()
    n_params = flat.numel()
    cases = [
        (dict(seeds=None), -1, "null pointer"),
        (dict(params=None), -1, "null pointer"),
        (dict(ws=None), -1, "null pointer"),
        (dict(loss=None), -1, "null pointer"),
        (dict(z=None), -1, "null pointer"),
        (dict(stats=None), -1, "null pointer"),
        (dict(layout=False), -1, "null pointer"),
        (dict(K=0), -1, "nbridges and lfsteps must be >= 1"),
        (dict(L=0), -1, "nbridges and lfsteps must be >= 1"),
        (dict(n=0), -1, "n or dim out of range"),
        (dict(ws_bytes=64), -3, "workspace too small"),
        (dict(target=LGCP, dim=1600), -2, "lgcp"),
        (dict(target=FUNNEL), -2, "no Hamiltonian AIS kernel instance"),        # funnel at dim 2
        (dict(dim=3), -2, "no Hamiltonian AIS kernel instance"),
        (dict(target=MANY_GMM), -1, "many_gmm needs target_consts"),
        (dict(target=MANY_GMM, consts=P, n_consts=4), -1, "many_gmm needs target_consts"),
        (dict(target=MANY_GMM, consts=P, n_consts=1 + 2 * 65), -1, "many_gmm needs target_consts"),
    ]
    for kw, status, text in cases:
        rc = call(hip_lib, lay, n_params, **kw)
        assert rc == status, (kw, rc, _lib.last_error())
        assert text in _lib.last_error(), (kw, _lib.last_error())
    # many_gmm with its constants gets as far as the workspace check
    assert call(hip_lib, lay, n_params, target=MANY_GMM, consts=P, n_consts=81, ws_bytes=64) == -3
    # every offset of the layout must lie inside params_flat
    for field in _lib.HAIS_LAYOUT_FIELDS[:-1]:
        for bad in (-1, n_params):
            broken = _lib.HaisLayout(**{f: getattr(lay, f) for f in _lib.HAIS_LAYOUT_FIELDS})
            setattr(broken, field, bad)
            assert call(hip_lib, broken, n_params) == -1 and "layout offset" in _lib.last_error(), (field, bad)
    assert call(hip_lib, lay, 10) == -1 and "layout offset" in _lib.last_error()
    broken = _lib.HaisLayout(**{f: getattr(lay, f) for f in _lib.HAIS_LAYOUT_FIELDS})
    broken.ngrid = -1
    assert call(hip_lib, broken, n_params) == -1 and "ngrid" in _lib.last_error()
    with pytest.raises(NotImplementedError):
        _lib.check(call(hip_lib, lay, n_params, target=LGCP, dim=1600))
    with pytest.raises(ValueError):
        _lib.check(call(hip_lib, lay, n_params, L=0))


def test_python_entry_points_validate_before_they_need_a_device(hip_lib):
    flat, un, fixed = hr.make_params(2, 8, 1, 0.05)
    gmm = model_handler.load_model("gmm")[0]
    wide = model_handler.load_model("funnel")[0]
    seeds = torch.arange(1, 9, dtype=torch.int32)
    assert hais.initialize is __import__("cmcd_amd.boundingmachine", fromlist=["initialize"]).initialize and fixed == (2, 8, 1)
    for fn in (hais.compute_bound, hais.grad_and_loss):
        with pytest.raises(RuntimeError, match="the CMCD hot path runs on a ROCm device only: params_flat is not a device tensor"):
            fn(seeds, flat, un, fixed, gmm)
        with pytest.raises(TypeError, match="log_prob must be a cmcd_amd.model_handler.Target"):
            fn(seeds, flat, un, fixed, lambda z: z.sum())
        with pytest.raises(ValueError, match="target dim 10 != params_fixed dim 2"):
            fn(seeds, flat, un, fixed, wide)
        with pytest.raises(ValueError, match="lfsteps"):
            fn(seeds, flat, un, (2, 8, 0), gmm)
        with pytest.raises(RuntimeError, match="runs on a ROCm device only"):      # nbridges = 0: the mean-field bound's own checks
            fn(seeds, flat, un, (2, 0, 1), gmm)
