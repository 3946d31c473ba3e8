"""cmcd_resample_systematic / cmcd_resample_workspace_bytes without a GPU: declared, exported, and every refusal decided on
the host before anything touches the device (all device pointers here are null or a dummy address that is never followed)."""
import ctypes as C
import os
import re

import pytest
import torch

from cmcd_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = C.c_void_p(16)        # "some non-null device pointer": a refused call never reads it


def call(lib, loss=P, z=None, n=64, dim=0, groups=1, seed=0, ws=None, ws_bytes=0, out_index=None, out_z=None, out_stats=P):
    return lib.cmcd_resample_systematic(loss, z, n, dim, groups, seed, ws, ws_bytes, out_index, out_z, out_stats, None)


def test_header_declares_and_library_exports_the_resampling_entry_points(hip_lib):
    src = open(os.path.join(ROOT, "include", "cmcd_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(cmcd_[a-z_0-9]+)\s*\(", src))
    for name in ("cmcd_resample_workspace_bytes", "cmcd_resample_systematic"):
        assert name in declared, f"{name} is not declared in include/cmcd_hip.h"
        assert hasattr(hip_lib, name), f"{name} is not exported"
    assert hip_lib.cmcd_version() == 3      # additive: the ABI version does not move


def test_refusals_are_decided_before_any_gpu_work(hip_lib):
    cases = [
        (dict(loss=None), -1, "null pointer"),
        (dict(out_stats=None), -1, "null pointer"),
        (dict(n=0), -1, "n out of range"),
        (dict(n=-5), -1, "n out of range"),
        (dict(groups=0), -1, "groups must be >= 1"),
        (dict(groups=-2), -1, "groups must be >= 1"),
        (dict(n=64, groups=3), -1, "multiple of groups"),
        (dict(out_z=P, z=None, dim=2), -1, "out_z needs z"),
        (dict(z=P, dim=0), -1, "dim must be >= 1"),
        (dict(z=P, out_z=P, dim=-1), -1, "dim must be >= 1"),
        (dict(n=(1 << 20) + 1), -2, "2^20"),
        (dict(n=2 * ((1 << 20) + 1), groups=2), -2, "2^20"),
    ]
    for kw, status, text in cases:
        rc = call(hip_lib, **kw)
        assert rc == status, (kw, rc, _lib.last_error())
        assert text in _lib.last_error(), (kw, _lib.last_error())
    with pytest.raises(ValueError):
        _lib.check(call(hip_lib, groups=0))
    with pytest.raises(NotImplementedError):
        _lib.check(call(hip_lib, n=(1 << 20) + 1))


def test_workspace_too_small_is_refused_with_the_shared_message(hip_lib):
    need = hip_lib.cmcd_resample_workspace_bytes(6000, 3)
    assert need > 0
    for ws, nbytes in ((None, 0), (P, need - 1), (C.c_void_p(24), need)):       # missing, short, not 16-byte aligned
        rc = call(hip_lib, n=6000, groups=3, ws=ws, ws_bytes=nbytes)
        assert rc == -3
        assert _lib.last_error() == f"workspace too small or not 16-byte aligned (need {need} bytes)"
    # the same form as the forward entry point's
    d = _lib.Desc(dim=2, nbridges=8, mode=0, arch=1, emb_dim=64, target=0, eps_schedule=0, grad_clipping=0, ngrid=8, reserved=0)
    lay = _lib.Layout(*([0] * len(_lib.LAYOUT_FIELDS)))
    rc = hip_lib.cmcd_bound_forward(C.byref(d), C.byref(lay), P, 16, P, 1 << 20, None, 0, P, 0, P, P, P, None)
    assert rc == -3
    assert re.fullmatch(r"workspace too small or not 16-byte aligned \(need \d+ bytes\)", _lib.last_error())


def test_size_query_is_positive_and_monotone(hip_lib):
    sizes = [hip_lib.cmcd_resample_workspace_bytes(n, 1) for n in (1, 2, 63, 64, 65, 1023, 1024, 1025, 15000, 1 << 20)]
    assert all(s > 0 and s % 16 == 0 for s in sizes)
    assert sizes == sorted(sizes) and sizes[-1] > sizes[0]
    assert all(s >= 12 * n for s, n in zip(sizes, (1, 2, 63, 64, 65, 1023, 1024, 1025, 15000, 1 << 20)))   # float64 sums + int32 ancestors
    assert hip_lib.cmcd_resample_workspace_bytes(60000, 30) == hip_lib.cmcd_resample_workspace_bytes(60000, 1)
    for n, groups in ((0, 1), (-1, 1), (10, 0), (10, 3), ((1 << 20) + 1, 1)):                              # what the call refuses
        assert hip_lib.cmcd_resample_workspace_bytes(n, groups) == 0


def test_python_entry_points_refuse_cpu_tensors(hip_lib):
    from cmcd_amd import resample, utils
    losses, z = torch.zeros(8), torch.zeros(8, 2)
    with pytest.raises(RuntimeError, match="runs on a ROCm device only"):
        resample.resample(losses, z)
    with pytest.raises(RuntimeError, match="runs on a ROCm device only"):
        resample.importance_stats(losses, groups=2)
    with pytest.raises(RuntimeError, match="runs on a ROCm device only"):
        utils.log_importance_diagnostics(losses.view(2, 4))
    assert resample.CHUNK == 1024 and resample.MAX_GROUP == 1 << 20
