"""The reverse-chain entry points of LDVI and UHA (include/cmcd_hip.h: cmcd_reverse_ldvi_workspace_bytes / cmcd_bound_reverse_ldvi,
cmcd_reverse_hais_workspace_bytes / cmcd_bound_reverse_hais) without a GPU: declared, exported, additive (the ABI version stays 3),
the size queries consistent with the calls, and every refusal decided on the host before anything touches the device (all device
pointers here are a dummy address that is never followed).  The older reverse entry points keep refusing these modes."""
import ctypes as C
import os
import re

import pytest
import torch

from cmcd_amd import _lib, build, hais, ldvi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = C.c_void_p(16)        # "some non-null device pointer": a refused call never reads it
GMM, FUNNEL, MANY, LGCP = 0, 1, 2, 3
GEFFNER, DDS = 0, 1
NAMES = ("cmcd_reverse_ldvi_workspace_bytes", "cmcd_bound_reverse_ldvi", "cmcd_reverse_hais_workspace_bytes", "cmcd_bound_reverse_hais")


def _desc(**kw):
    base = dict(dim=2, nbridges=8, mode=0, arch=GEFFNER, emb_dim=20, target=GMM, eps_schedule=0, grad_clipping=0, ngrid=8, reserved=0)
    base.update(kw)
    return _lib.Desc(**base)


def test_header_declares_and_library_exports_the_entry_points(hip_lib):
    src = open(os.path.join(ROOT, "include", "cmcd_hip.h")).read()
    assert "m_f   = rho_i (1 - eta) " in src and "r   = eta rho + sqrt(1 - eta^2) s xi_r" in src      # the arithmetic is written out
    assert "no reverse chain for LDVI" not in src
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(cmcd_[a-z_0-9]+)\s*\(", src))
    for name in NAMES:
        assert name in declared, f"{name} is not declared in include/cmcd_hip.h"
        assert hasattr(hip_lib, name), f"{name} is not exported"
    assert hip_lib.cmcd_version() == 3      # additive: the ABI version does not move
    for f in ("cmcd_reverse_ldvi.hip", "cmcd_reverse_hais.hip"):
        assert f in build.SOURCES and build.EXTRA_FLAGS[f] == ["-fno-slp-vectorize"]


# ------------------------------------------------------------------------------------------ LDVI
def ldvi_setup(mode="MCD_U_a-lp-sn", **kw):
    flat, un, fixed = ldvi.initialize(2, nbridges=8, eps=0.01, emb_dim=20, mode=mode, nn_arch="geffner", device="cpu",
                                      trainable=("eta", "gamma", "eps", "vd", "mgridref_y"), **kw)
    from cmcd_amd.model_handler import load_model
    desc, lay, use_net = ldvi._plan(un, fixed, load_model("gmm")[0])
    return flat, desc, lay, use_net


def ldvi_call(lib, flat, desc, lay, use_net, seeds=P, x=P, n=32, params=P, ws=P, ws_bytes=1 << 40, w=P, z0=P, rho0=P, stats=P,
              consts=None, n_consts=0, n_params=None):
    return lib.cmcd_bound_reverse_ldvi(C.byref(desc), C.byref(lay), use_net, seeds, x, n, params,
                                       flat.numel() if n_params is None else n_params, consts, n_consts, ws, ws_bytes, w, z0, rho0,
                                       stats, None)


def test_ldvi_size_query(hip_lib):
    q, fq = hip_lib.cmcd_reverse_ldvi_workspace_bytes, hip_lib.cmcd_ldvi_workspace_bytes
    for kw, use_net, n in ((dict(), 1, 300), (dict(), 0, 33), (dict(emb_dim=40), 1, 1), (dict(target=MANY), 1, 2000),
                           (dict(target=FUNNEL, dim=10, emb_dim=48), 1, 17), (dict(target=FUNNEL, dim=10), 0, 17)):
        need = q(C.byref(_desc(**kw)), use_net, n)
        assert need > 0 and need % 16 == 0 and need == fq(C.byref(_desc(**kw)), use_net, n, 0), (kw, use_net, n)
    # the descriptor's mode, schedule, clip and kernel variant are ignored
    assert q(C.byref(_desc(mode=9, eps_schedule=2, grad_clipping=1, reserved=3)), 1, 300) == q(C.byref(_desc()), 1, 300)
    assert q(None, 1, 300) == 0
    for n in (0, -5):
        assert q(C.byref(_desc()), 1, n) == 0


@pytest.mark.parametrize("kw,use_net,msg", [
    (dict(target=LGCP, dim=1600), 1, "lgcp"),
    (dict(target=LGCP, dim=1600), 0, "lgcp"),
    (dict(arch=DDS, emb_dim=64), 1, "nn_arch"),                              # the dds arch
    (dict(emb_dim=130), 1, "kernel instance"),                               # 134 wide: 9 tiles, no instance
    (dict(target=FUNNEL, dim=10, emb_dim=12), 1, "kernel instance"),         # the funnel on 2 tiles ...
    (dict(target=FUNNEL, dim=10, emb_dim=100), 1, "kernel instance"),        # ... and on 9
    (dict(nbridges=5000), 1, "nbridges above 4096"),
])
def test_ldvi_unsupported_configurations(hip_lib, kw, use_net, msg):
    d = _desc(**kw)
    assert hip_lib.cmcd_reverse_ldvi_workspace_bytes(C.byref(d), use_net, 300) == 0
    assert msg in _lib.last_error()
    lay = _lib.Layout(*([-1] * len(_lib.LAYOUT_FIELDS)))
    rc = hip_lib.cmcd_bound_reverse_ldvi(C.byref(d), C.byref(lay), use_net, None, None, 300, None, 0, None, 0, None, 0, None, None,
                                         None, None, None)
    assert rc == -2 and msg in _lib.last_error()      # refused before the pointers are looked at
    with pytest.raises(NotImplementedError, match=msg):
        _lib.check(rc)


@pytest.mark.parametrize("mode", ["MCD_U_a-lp-sn", "MCD_U_a-lp"])
def test_ldvi_refusals_are_decided_before_any_gpu_work(hip_lib, mode):
    flat, desc, lay, use_net = ldvi_setup(mode)
    need = hip_lib.cmcd_reverse_ldvi_workspace_bytes(C.byref(desc), use_net, 32)
    assert need > 0
    cases = [(dict(**{k: None}), -1, "null pointer") for k in ("seeds", "x", "params", "ws", "w", "z0", "rho0", "stats")] + [
        (dict(n=0), -1, "n out of range"),
        (dict(n=-5), -1, "n out of range"),
        (dict(ws_bytes=need - 1), -3, "workspace too small"),
        (dict(ws=C.c_void_p(24)), -3, "16-byte aligned"),
        (dict(n_params=10), -1, "layout offset"),
    ]
    for kw, status, text in cases:
        rc = ldvi_call(hip_lib, flat, desc, lay, use_net, **kw)
        assert rc == status, (kw, rc, _lib.last_error())
        assert text in _lib.last_error(), (kw, _lib.last_error())
    with pytest.raises(ValueError):
        _lib.check(ldvi_call(hip_lib, flat, desc, lay, use_net, x=None))
    many = _desc(target=MANY)      # many_gmm without its constants
    assert hip_lib.cmcd_bound_reverse_ldvi(C.byref(many), C.byref(lay), use_net, P, P, 32, P, flat.numel(), None, 0, P, 1 << 40, P, P, P,
                                           P, None) == -1 and "many_gmm needs target_consts" in _lib.last_error()


# ------------------------------------------------------------------------------------------ UHA
def hais_setup(dim=2, K=8, L=1):
    flat, un, fixed = hais.initialize(dim=dim, nbridges=K, lfsteps=L, eps=0.05, eta=0.5, device="cpu",
                                      trainable=("eta", "eps", "vd", "mgridref_y"))
    return flat, hais._layout(un)


def hais_call(lib, flat, lay, target=GMM, dim=2, K=8, L=1, seeds=P, x=P, n=32, params=P, ws=P, ws_bytes=1 << 40, w=P, z0=P, rho0=P,
              stats=P, consts=None, n_consts=0, n_params=None, layout=True):
    return lib.cmcd_bound_reverse_hais(target, dim, K, L, lay if layout else None, seeds, x, n, params,
                                       flat.numel() if n_params is None else n_params, consts, n_consts, ws, ws_bytes, w, z0, rho0, stats,
                                       None)


def test_hais_size_query(hip_lib):
    q = hip_lib.cmcd_reverse_hais_workspace_bytes
    rec = lambda tiles: (tiles * 10 + 3) // 4 * 16      # one 5-double record per 16-particle tile, rounded up to 16 bytes
    assert q(GMM, 2, 8, 1, 1) == rec(1) == 48 and q(GMM, 2, 8, 3, 17) == rec(2) == 80 and q(MANY, 2, 256, 1, 2000) == rec(125)
    assert q(FUNNEL, 10, 64, 2, 300) == rec(19)
    assert q(GMM, 2, 4096, 4096, 16) > 0                                    # nbridges * lfsteps = 2^24: the limit itself
    for args, text in (((GMM, 2, 0, 1, 32), "nbridges and lfsteps"), ((GMM, 2, -1, 1, 32), "nbridges and lfsteps"),
                       ((GMM, 2, 8, 0, 32), "nbridges and lfsteps"), ((GMM, 2, 8, 1, 0), "n or dim"), ((GMM, 2, 8, 1, -5), "n or dim"),
                       ((GMM, 0, 8, 1, 32), "n or dim"), ((LGCP, 1600, 8, 1, 32), "lgcp"), ((GMM, 3, 8, 1, 32), "kernel instance"),
                       ((FUNNEL, 2, 8, 1, 32), "kernel instance"), ((GMM, 2, 4097, 1, 32), "nbridges above 4096"),
                       ((GMM, 2, 4096, 4097, 32), "2^24")):
        assert q(*args) == 0 and text in _lib.last_error(), (args, _lib.last_error())


def test_hais_refusals_are_decided_before_any_gpu_work(hip_lib):
    flat, lay = hais_setup()
    need = hip_lib.cmcd_reverse_hais_workspace_bytes(GMM, 2, 8, 1, 32)
    cases = [(dict(**{k: None}), -1, "null pointer") for k in ("seeds", "x", "params", "ws", "w", "z0", "rho0", "stats")] + [
        (dict(layout=False), -1, "null pointer"),
        (dict(n=0), -1, "n or dim out of range"),
        (dict(n=-5), -1, "n or dim out of range"),
        (dict(K=0), -1, "nbridges and lfsteps must be >= 1"),
        (dict(K=-3), -1, "nbridges and lfsteps must be >= 1"),
        (dict(L=0), -1, "nbridges and lfsteps must be >= 1"),
        (dict(K=4097), -2, "nbridges above 4096"),
        (dict(K=4096, L=4097), -2, "2^24"),
        (dict(target=LGCP, dim=1600), -2, "lgcp"),
        (dict(dim=3), -2, "kernel instance"),
        (dict(target=FUNNEL), -2, "kernel instance"),                        # the funnel at dim 2
        (dict(ws_bytes=need - 1), -3, "workspace too small"),
        (dict(ws=C.c_void_p(24)), -3, "16-byte aligned"),
        (dict(n_params=10), -1, "layout offset"),
        (dict(target=MANY), -1, "many_gmm needs target_consts"),
    ]
    for kw, status, text in cases:
        rc = hais_call(hip_lib, flat, lay, **kw)
        assert rc == status, (kw, rc, _lib.last_error())
        assert text in _lib.last_error(), (kw, _lib.last_error())
    with pytest.raises(NotImplementedError, match="lgcp"):
        _lib.check(hais_call(hip_lib, flat, lay, target=LGCP, dim=1600))
    with pytest.raises(ValueError):
        _lib.check(hais_call(hip_lib, flat, lay, x=None))
    big =_lib.HaisLayout(**{k: getattr(lay, k) for k in _lib.HAIS_LAYOUT_FIELDS})
    big.ngrid = 2000
    assert hais_call(hip_lib, flat, big) == -1 and "ngrid out of range" in _lib.last_error()


# ------------------------------------------------------------------------------------------ the older entry points
def test_the_older_reverse_entry_points_keep_refusing_these_modes(hip_lib):
    """cmcd_bound_reverse has no momentum; cmcd_bound_reverse_uha is the 2nd-order chain (two network evaluations per bridge, the cos^2
    table, the clip).  Neither has a mode value for LDVI or UHA: the descriptor LDVI hands the library carries MCD_CAIS_UHA_sn's value as
    a placeholder, which cmcd_bound_reverse refuses; a mode value past the table is refused by both; and the Python modules refuse the
    strings."""
    from cmcd_amd import mcdboundingmachine as mcdbm
    from cmcd_amd import reverse_uha
    from cmcd_amd.model_handler import load_model
    flat, desc, lay, use_net = ldvi_setup()
    assert hip_lib.cmcd_reverse_workspace_bytes(C.byref(desc), 32) == 0 and "overdamped modes only" in _lib.last_error()
    for q in (hip_lib.cmcd_reverse_workspace_bytes, hip_lib.cmcd_reverse_uha_workspace_bytes):
        assert q(C.byref(_desc(mode=5)), 32) == 0 and "Mode not implemented" in _lib.last_error()
    tgt = load_model("gmm")[0]
    seeds, x = torch.arange(1, 33, dtype=torch.int32), torch.zeros(32, 2)
    for mode in ("MCD_U_a-lp-sn", "MCD_U_a-lp"):
        f, un, fixed = ldvi.initialize(2, nbridges=8, eps=0.01, emb_dim=20, mode=mode, nn_arch="geffner", device="cpu")
        for fn in (mcdbm.bound_reverse, reverse_uha.bound_reverse):
            with pytest.raises(NotImplementedError, match="Mode not implemented"):
                fn(seeds, x, f, un, fixed, tgt)
    f, un, fixed = hais.initialize(dim=2, nbridges=8, lfsteps=1, eps=0.05, eta=0.5, device="cpu")
    for fn in (mcdbm.bound_reverse, reverse_uha.bound_reverse):
        with pytest.raises((NotImplementedError, ValueError)):      # params_fixed = (dim, nbridges, lfsteps): no mode string at all
            fn(seeds, x, f, un, fixed, tgt)


def test_python_entry_points_refuse_host_tensors(hip_lib):
    from cmcd_amd import reverse_hais, reverse_ldvi
    from cmcd_amd.model_handler import load_model
    assert reverse_ldvi.__all__ == ["bound_reverse", "compute_reverse_bound"] == reverse_hais.__all__
    tgt = load_model("gmm")[0]
    seeds = torch.arange(1, 33, dtype=torch.int32)
    f, un, fixed = ldvi.initialize(2, nbridges=8, eps=0.01, emb_dim=20, mode="MCD_U_a-lp-sn", nn_arch="geffner", device="cpu")
    for fn in (reverse_ldvi.bound_reverse, reverse_ldvi.compute_reverse_bound):
        with pytest.raises(RuntimeError, match="runs on a ROCm device only"):
            fn(seeds, torch.zeros(32, 2), f, un, fixed, tgt)
    f, un, fixed = hais.initialize(dim=2, nbridges=8, lfsteps=1, eps=0.05, eta=0.5, device="cpu")
    for fn in (reverse_hais.bound_reverse, reverse_hais.compute_reverse_bound):
        with pytest.raises(RuntimeError, match="runs on a ROCm device only"):
            fn(seeds, torch.zeros(32, 2), f, un, fixed, tgt)
    with pytest.raises(ValueError, match="nbridges"):
        reverse_hais.bound_reverse(seeds, torch.zeros(32, 2), f, un, (2, 0, 1), tgt)
