"""The LDVI entry points of the C ABI (include/cmcd_hip.h: cmcd_ldvi_workspace_bytes, cmcd_ldvi_bound_grad): exported, additive
(the ABI version stays 3), and every refusal answered before any GPU work — codes, messages and order as the sibling entry points."""
import ctypes as C

import numpy as np
import pytest
import torch

from cmcd_amd import _lib, ldvi
from cmcd_amd import mcdboundingmachine as mcdbm

GMM, FUNNEL, MANY, LGCP = 0, 1, 2, 3
GEFFNER, DDS = 0, 1


def _desc(**kw):
    base = dict(dim=2, nbridges=8, mode=0, arch=GEFFNER, emb_dim=20, target=GMM, eps_schedule=0, grad_clipping=0, ngrid=8, reserved=0)
    base.update(kw)
    return _lib.Desc(**base)


def test_symbols_are_exported_and_the_version_stays(hip_lib):
    assert hasattr(hip_lib, "cmcd_ldvi_workspace_bytes") and hasattr(hip_lib, "cmcd_ldvi_bound_grad")
    assert hip_lib.cmcd_version() == 3


def test_size_query(hip_lib):
    q = hip_lib.cmcd_ldvi_workspace_bytes
    fwd, grad = q(C.byref(_desc()), 1, 300, 0), q(C.byref(_desc()), 1, 300, 1)
    assert fwd > 0 and fwd % 16 == 0 and grad > fwd and grad % 16 == 0
    # what a gradient call keeps: 4 K + 2 rows of n dim floats, and more
    assert grad - fwd >= (4 * 8 + 2) * 300 * 2 * 4
    assert q(C.byref(_desc()), 1, 600, 1) > grad
    # the descriptor's mode, schedule, clip and kernel variant are ignored
    assert q(C.byref(_desc(mode=9, eps_schedule=2, grad_clipping=1, reserved=3)), 1, 300, 1) == grad
    # without a network: smaller, and the architecture field is not read
    nonet = q(C.byref(_desc()), 0, 300, 1)
    assert 0 < nonet < grad and q(C.byref(_desc(arch=DDS, emb_dim=64)), 0, 300, 1) == nonet
    # instances: gmm / many_gmm on 2 and 4 neuron tiles, the funnel (d = 10) on 5
    assert q(C.byref(_desc(target=MANY)), 1, 2000, 1) > 0
    assert q(C.byref(_desc(emb_dim=40)), 1, 300, 1) > 0                      # 44 wide -> 4 tiles
    assert q(C.byref(_desc(target=FUNNEL, dim=10, emb_dim=48)), 1, 300, 1) > 0
    assert q(C.byref(_desc(target=FUNNEL, dim=10)), 0, 300, 1) > 0


@pytest.mark.parametrize("kw,use_net,msg", [
    (dict(target=LGCP, dim=1600), 1, "lgcp"),
    (dict(target=LGCP, dim=1600), 0, "lgcp"),
    (dict(arch=DDS, emb_dim=64), 1, "nn_arch"),
    (dict(emb_dim=130), 1, "no LDVI kernel instance"),                       # 134 wide: 9 tiles, no instance
    (dict(target=FUNNEL, dim=10, emb_dim=100), 1, "no LDVI kernel instance"),   # d = 10 on 9 tiles
    (dict(target=FUNNEL, dim=4), 0, "instance"),                             # a funnel of another dimension
    (dict(nbridges=5000), 1, "nbridges above 4096"),
])
def test_unsupported_configurations(hip_lib, kw, use_net, msg):
    d = _desc(**kw)
    assert hip_lib.cmcd_ldvi_workspace_bytes(C.byref(d), use_net, 300, 1) == 0
    assert msg in _lib.last_error()
    lay = _lib.Layout(*([-1] * len(_lib.LAYOUT_FIELDS)))
    rc = hip_lib.cmcd_ldvi_bound_grad(C.byref(d), C.byref(lay), use_net, None, 300, None, 0, None, 0, 1.0, None, 0, None, None,
                                      None, None, None)
    assert rc == -2 and msg in _lib.last_error()      # refused before the pointers are looked at
    with pytest.raises(NotImplementedError, match=msg):
        _lib.check(rc)


def test_bad_descriptor_values(hip_lib):
    q = hip_lib.cmcd_ldvi_workspace_bytes
    assert q(None, 1, 300, 1) == 0
    assert q(C.byref(_desc(nbridges=0)), 1, 300, 1) == 0 and "nbridges" in _lib.last_error()
    assert q(C.byref(_desc(ngrid=40)), 1, 300, 1) == 0 and "ngrid" in _lib.last_error()
    for n in (0, -5):
        assert q(C.byref(_desc()), 1, n, 1) == 0


def _call_args(mode="MCD_U_a-lp-sn", n=33):
    """Host buffers standing in for the device ones: every refusal below is answered before anything is launched."""
    flat, un, fixed = ldvi.initialize(2, nbridges=8, eps=0.01, emb_dim=20, mode=mode, nn_arch="geffner", device="cpu",
                                      trainable=("eta", "gamma", "eps", "vd", "mgridref_y"))
    use_net = int(mode == "MCD_U_a-lp-sn")
    lay = mcdbm._layout(un, fixed[3]) if use_net else mcdbm._layout_no_net(un)
    lay.gamma = un.offset("gamma")
    d = _desc(ngrid=un.shape("mgridref_y")[0] - 1)
    seeds = torch.arange(1, n + 1, dtype=torch.int32)
    loss, z, stats = torch.zeros(n), torch.zeros(n, 2), torch.zeros(5, dtype=torch.float64)
    return d, lay, use_net, seeds, flat, loss, z, stats


@pytest.mark.parametrize("mode", ldvi.MODES)
def test_argument_refusals_before_any_gpu_work(hip_lib, mode):
    d, lay, use_net, seeds, flat, loss, z, stats = _call_args(mode)
    n = seeds.numel()
    need = hip_lib.cmcd_ldvi_workspace_bytes(C.byref(d), use_net, n, 1)
    assert need > 0
    ws = torch.zeros(need + 64, dtype=torch.uint8)
    base = (ws.data_ptr() + 15) & ~15
    grad = torch.zeros_like(flat)

    def call(n=n, lay=lay, ws_ptr=base, ws_bytes=need, seeds_ptr=seeds.data_ptr(), n_params=flat.numel(), grad_ptr=grad.data_ptr()):
        return hip_lib.cmcd_ldvi_bound_grad(C.byref(d), C.byref(lay), use_net, seeds_ptr, n, flat.data_ptr(), n_params, None, 0,
                                            1.0 / 33, ws_ptr, ws_bytes, loss.data_ptr(), z.data_ptr(), stats.data_ptr(), grad_ptr,
                                            None)

    assert call(seeds_ptr=None) == -1 and "null pointer" in _lib.last_error()
    for bad_n in (0, -3):
        assert call(n=bad_n) == -1 and "n out of range" in _lib.last_error()
    empty = _lib.Layout(*([-1] * len(_lib.LAYOUT_FIELDS)))
    assert call(lay=empty) == -1 and "layout offset" in _lib.last_error()
    no_gamma = _lib.Layout.from_buffer_copy(bytes(lay))
    no_gamma.gamma = -1
    assert call(lay=no_gamma) == -1 and "layout offset" in _lib.last_error()
    assert call(n_params=lay.mgridref_y + 1) == -1 and "layout offset" in _lib.last_error()   # params_flat ends inside a leaf
    assert call(ws_bytes=need - 1) == -3 and "workspace" in _lib.last_error()
    assert call(ws_ptr=base + 4) == -3 and "16-byte aligned" in _lib.last_error()
    # a forward-only call asks for the forward size only
    fwd = hip_lib.cmcd_ldvi_workspace_bytes(C.byref(d), use_net, n, 0)
    assert call(ws_bytes=fwd - 1, grad_ptr=None) == -3
    with pytest.raises(RuntimeError):
        _lib.check(-3)


def test_many_gmm_needs_its_constants(hip_lib):
    d, lay, use_net, seeds, flat, loss, z, stats = _call_args()
    d.target = MANY
    rc = hip_lib.cmcd_ldvi_bound_grad(C.byref(d), C.byref(lay), use_net, seeds.data_ptr(), seeds.numel(), flat.data_ptr(),
                                      flat.numel(), None, 0, 1.0, flat.data_ptr(), 1 << 30, loss.data_ptr(), z.data_ptr(),
                                      stats.data_ptr(), None, None)
    assert rc == -1 and "many_gmm needs target_consts" in _lib.last_error()
    assert np.all(loss.numpy() == 0)
