"""cmcd_sinkhorn_workspace_bytes / _setup / _iterate / _cost without a GPU: declared, exported, the size query against the formula
written in include/cmcd_hip.h, and every refusal decided on the host before anything touches the device (all device pointers
here are null or a dummy address that is never followed)."""
import ctypes as C
import os
import re

import pytest
import torch

from cmcd_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = C.c_void_p(16)        # "some non-null device pointer": a refused call never reads it
NAMES = ("cmcd_sinkhorn_workspace_bytes", "cmcd_sinkhorn_setup", "cmcd_sinkhorn_iterate", "cmcd_sinkhorn_cost")


def setup(lib, x=P, y=P, a=None, b=None, n=64, dim=2, groups=3, reg=0.01, ws=P, ws_bytes=1 << 40):
    return lib.cmcd_sinkhorn_setup(x, y, a, b, n, dim, groups, reg, ws, ws_bytes, None)


def iterate(lib, n=64, dim=2, groups=3, first=0, count=10, cap=100, thr=1e-16, ws=P, ws_bytes=1 << 40, flags=None):
    return lib.cmcd_sinkhorn_iterate(n, dim, groups, first, count, cap, thr, ws, ws_bytes, flags, None)


def cost(lib, x=P, y=P, n=64, dim=2, groups=3, ws=P, ws_bytes=1 << 40, out=P, flags=None):
    return lib.cmcd_sinkhorn_cost(x, y, n, dim, groups, ws, ws_bytes, out, flags, None)


def formula(n, groups):
    """include/cmcd_hip.h: bytes = 32 groups + 8 (groups n^2 + 5 groups n + 2 groups T n + groups T), T = ceil(n / 64),
    rounded up to a multiple of 16"""
    T = (n + 63) // 64
    nbytes = 32 * groups + 8 * (groups * n * n + 5 * groups * n + 2 * groups * T * n + groups * T)
    return (nbytes + 15) // 16 * 16


def test_header_declares_and_library_exports_the_entry_points(hip_lib):
    src = open(os.path.join(ROOT, "include", "cmcd_hip.h")).read()
    assert "32 groups + 8 (groups n^2 + 5 groups n + 2 groups T n + groups T)" in src      # the formula `formula` restates
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(cmcd_[a-z_0-9]+)\s*\(", src))
    for name in NAMES:
        assert name in declared, f"{name} is not declared in include/cmcd_hip.h"
        assert hasattr(hip_lib, name), f"{name} is not exported"
    assert hip_lib.cmcd_version() == 3      # additive: the ABI version does not move


@pytest.mark.parametrize("n,dim,groups", [(2, 1, 1), (65, 10, 3), (500, 2, 120), (8192, 2, 1), (63, 65, 7)])
def test_size_query_is_the_formula_of_the_header(hip_lib, n, dim, groups):
    got = hip_lib.cmcd_sinkhorn_workspace_bytes(n, dim, groups)
    assert got == formula(n, groups) and got % 16 == 0
    assert got >= 8 * groups * n * n


def test_size_query_answers_zero_to_what_the_calls_refuse(hip_lib):
    for n, dim, groups in ((1, 2, 1), (0, 2, 1), (-3, 2, 1), (8193, 2, 1), (64, 0, 1), (64, 2, 0), (64, 2, -1), (64, 2, 65536)):
        assert hip_lib.cmcd_sinkhorn_workspace_bytes(n, dim, groups) == 0, (n, dim, groups)


def test_refusals_are_decided_before_any_gpu_work(hip_lib):
    shape = [
        (dict(n=1), -1, "n must be >= 2"),
        (dict(n=0), -1, "n must be >= 2"),
        (dict(dim=0), -1, "dim must be >= 1"),
        (dict(groups=0), -1, "groups must be >= 1"),
        (dict(groups=-2), -1, "groups must be >= 1"),
        (dict(n=8193), -2, "8192"),
        (dict(groups=65536), -2, "65535"),
    ]
    for fn in (setup, iterate, cost):
        for kw, status, text in shape:
            rc = fn(hip_lib, **kw)
            assert rc == status, (fn.__name__, kw, rc, _lib.last_error())
            assert text in _lib.last_error(), (fn.__name__, kw, _lib.last_error())
    own = [
        (setup, dict(x=None), -1, "null pointer"),
        (setup, dict(y=None), -1, "null pointer"),
        (setup, dict(reg=0.0), -1, "reg must be positive"),
        (setup, dict(reg=float("nan")), -1, "reg must be positive"),
        (setup, dict(reg=float("inf")), -1, "reg must be positive"),
        (cost, dict(x=None), -1, "null pointer"),
        (cost, dict(y=None), -1, "null pointer"),
        (cost, dict(out=None), -1, "null pointer"),
        (iterate, dict(cap=0), -1, "num_iter_max"),
        (iterate, dict(first=-1), -1, "iterations must lie"),
        (iterate, dict(count=-1), -1, "iterations must lie"),
        (iterate, dict(first=95, count=10), -1, "iterations must lie"),
    ]
    for fn, kw, status, text in own:
        rc = fn(hip_lib, **kw)
        assert rc == status, (fn.__name__, kw, rc, _lib.last_error())
        assert text in _lib.last_error(), (fn.__name__, kw, _lib.last_error())
    with pytest.raises(ValueError):
        _lib.check(setup(hip_lib, n=1))
    with pytest.raises(NotImplementedError):
        _lib.check(setup(hip_lib, n=8193))


def test_workspace_too_small_is_refused_with_the_shared_message(hip_lib):
    need = hip_lib.cmcd_sinkhorn_workspace_bytes(64, 2, 3)
    assert need > 0
    for fn in (setup, iterate, cost):
        for ws, nbytes in ((None, 0), (P, need - 1), (C.c_void_p(24), need)):       # missing, short, not 16-byte aligned
            rc = fn(hip_lib, ws=ws, ws_bytes=nbytes)
            assert rc == -3, (fn.__name__, rc)
            assert _lib.last_error() == f"workspace too small or not 16-byte aligned (need {need} bytes)"


def test_python_entry_points_refuse_cpu_tensors(hip_lib):
    from cmcd_amd import sinkhorn, utils
    x = torch.zeros(2, 8, 2)
    with pytest.raises(RuntimeError, match="runs on a ROCm device only"):
        sinkhorn.w2_batched(x, x)
    with pytest.raises(RuntimeError, match="runs on a ROCm device only"):
        utils.calculate_W2_distances(x.view(16, 2), x.view(16, 2), x.view(16, 2), 8, 2, 8, batched=True)
    with pytest.raises(RuntimeError, match="runs on a ROCm device only"):
        utils.calculate_W2_distances(x.view(16, 2), x.view(16, 2), x.view(16, 2), 8, 2, 8, losses=torch.zeros(16))
    assert sinkhorn.ROWS == 64 and sinkhorn.MAX_N == 8192
