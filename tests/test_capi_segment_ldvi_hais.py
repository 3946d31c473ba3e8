"""The segment entry points of LDVI and UHA (include/cmcd_hip.h: cmcd_segment_ldvi_workspace_bytes / cmcd_bound_segment_ldvi,
cmcd_segment_hais_workspace_bytes / cmcd_bound_segment_hais) without a GPU: declared, exported, additive (the ABI version stays 3),
the size queries consistent with the calls and zero for everything the calls refuse, and every refusal decided on the host before
anything touches the device (all device pointers here are a dummy address that is never followed).  Modelled on
tests/test_capi_segment_uha.py and tests/test_capi_reverse_ldvi_hais.py."""
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
NAMES = ("cmcd_segment_ldvi_workspace_bytes", "cmcd_bound_segment_ldvi", "cmcd_segment_hais_workspace_bytes", "cmcd_bound_segment_hais")
RANGE = "0 <= k0 < k1 <= nbridges"


def _desc(**kw):
    base = dict(dim=2, nbridges=8, mode=0, arch=GEFFNER, emb_dim=20, target=GMM, eps_schedule=0, grad_clipping=0, ngrid=8, reserved=0)
    base.update(kw)
    return _lib.Desc(**base)


def test_header_declares_and_library_exports_the_entry_points(hip_lib):
    src = open(os.path.join(ROOT, "include", "cmcd_hip.h")).read()
    # the arithmetic is written out: LDVI's network-free forward mean, UHA's lg without a momentum term and why
    assert "m_f = rho (1 - eta)   " in src and "lg = log gamma_k1(z) alone, no momentum term" in src
    assert "the momentum densities telescope" in src and "must move rho with z" in src
    assert "no LDVI / UHA-boundmode segments" not in src
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(cmcd_[a-z_0-9]+)\s*\(", src))
    for name in NAMES:
        assert name in declared, f"{name} is not declared in include/cmcd_hip.h"
        assert hasattr(hip_lib, name), f"{name} is not exported"
    assert hip_lib.cmcd_version() == 3      # additive: the ABI version does not move
    for f in ("cmcd_segment_ldvi.hip", "cmcd_segment_hais.hip"):
        assert f in build.SOURCES and build.EXTRA_FLAGS[f] == ["-fno-slp-vectorize"]


# ------------------------------------------------------------------------------------------ LDVI
def ldvi_setup(mode="MCD_U_a-lp-sn", **kw):
    flat, un, fixed = ldvi.initialize(2, nbridges=8, eps=0.01, emb_dim=20, mode=mode, nn_arch="geffner", device="cpu",
                                      trainable=("eta", "gamma", "eps", "vd", "mgridref_y"), **kw)
    from cmcd_amd.model_handler import load_model
    desc, lay, use_net = ldvi._plan(un, fixed, load_model("gmm")[0])
    return flat, desc, lay, use_net


def ldvi_call(lib, flat, desc, lay, use_net, k0=0, k1=2, seeds=P, n=32, params=P, ws=P, ws_bytes=1 << 40, z=P, rho=P, wpath=P, key=P,
              lg=P, stats=P, consts=None, n_consts=0, n_params=None):
    return lib.cmcd_bound_segment_ldvi(C.byref(desc), C.byref(lay), use_net, k0, k1, seeds, n, params,
                                       flat.numel() if n_params is None else n_params, consts, n_consts, ws, ws_bytes, z, rho, wpath,
                                       key, lg, stats, None)


def test_ldvi_size_query_is_the_forward_layout(hip_lib):
    q, fq = hip_lib.cmcd_segment_ldvi_workspace_bytes, hip_lib.cmcd_ldvi_workspace_bytes
    for kw, use_net, n in ((dict(), 1, 300), (dict(), 0, 33), (dict(emb_dim=40), 1, 1), (dict(target=MANY), 1, 2000),
                           (dict(target=FUNNEL, dim=10, emb_dim=48), 1, 17), (dict(target=FUNNEL, dim=10), 0, 17)):
        need = q(C.byref(_desc(**kw)), use_net, n)
        assert need > 0 and need % 16 == 0 and need == fq(C.byref(_desc(**kw)), use_net, n, 0), (kw, use_net, n)
        assert need == hip_lib.cmcd_reverse_ldvi_workspace_bytes(C.byref(_desc(**kw)), use_net, n)
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
def test_ldvi_size_query_answers_zero_to_what_the_call_refuses(hip_lib, kw, use_net, msg):
    d = _desc(**kw)
    assert hip_lib.cmcd_segment_ldvi_workspace_bytes(C.byref(d), use_net, 300) == 0
    assert msg in _lib.last_error()
    lay = _lib.Layout(*([-1] * len(_lib.LAYOUT_FIELDS)))
    rc = hip_lib.cmcd_bound_segment_ldvi(C.byref(d), C.byref(lay), use_net, 0, 2, None, 300, None, 0, None, 0, None, 0, None, None,
                                         None, None, None, None, None)
    assert rc == -2 and msg in _lib.last_error()      # refused before the pointers are looked at
    with pytest.raises(NotImplementedError, match=msg):
        _lib.check(rc)


@pytest.mark.parametrize("mode", ["MCD_U_a-lp-sn", "MCD_U_a-lp"])
def test_ldvi_refusals_are_decided_before_any_gpu_work(hip_lib, mode):
    flat, desc, lay, use_net = ldvi_setup(mode)          # K = 8
    need = hip_lib.cmcd_segment_ldvi_workspace_bytes(C.byref(desc), use_net, 32)
    assert need > 0
    cases = [(dict(**{k: None}), -1, "null pointer") for k in ("params", "ws", "z", "rho", "wpath", "key", "lg", "stats")] + [
        (dict(rho=None, k0=1), -1, "null pointer"),
        (dict(k0=-1), -1, RANGE), (dict(k0=2, k1=2), -1, RANGE), (dict(k0=3, k1=2), -1, RANGE), (dict(k1=9), -1, RANGE),
        (dict(k0=8, k1=9), -1, RANGE),
        (dict(seeds=None), -1, "needs seeds"),
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
    # a null seeds pointer is fine past bridge 0: the call gets as far as the workspace check; so does the last bridge alone
    assert ldvi_call(hip_lib, flat, desc, lay, use_net, k0=1, k1=2, seeds=None, ws_bytes=64) == -3
    assert ldvi_call(hip_lib, flat, desc, lay, use_net, k0=7, k1=8, ws_bytes=need - 1) == -3
    with pytest.raises(ValueError):
        _lib.check(ldvi_call(hip_lib, flat, desc, lay, use_net, k1=9))
    many = _desc(target=MANY)      # many_gmm without its constants
    assert hip_lib.cmcd_bound_segment_ldvi(C.byref(many), C.byref(lay), use_net, 0, 2, P, 32, P, flat.numel(), None, 0, P, 1 << 40, P, P,
                                           P, P, P, P, None) == -1 and "many_gmm needs target_consts" in _lib.last_error()


# ------------------------------------------------------------------------------------------ UHA
def hais_setup(dim=2, K=8, L=1):
    flat, un, fixed = hais.initialize(dim=dim, nbridges=K, lfsteps=L, eps=0.05, eta=0.5, device="cpu",
                                      trainable=("eta", "eps", "vd", "mgridref_y"))
    return flat, hais._layout(un)


def hais_call(lib, flat, lay, target=GMM, dim=2, K=8, L=1, k0=0, k1=2, seeds=P, n=32, params=P, ws=P, ws_bytes=1 << 40, z=P, rho=P,
              wpath=P, key=P, lg=P, stats=P, consts=None, n_consts=0, n_params=None, layout=True):
    return lib.cmcd_bound_segment_hais(target, dim, K, L, lay if layout else None, k0, k1, seeds, n, params,
                                       flat.numel() if n_params is None else n_params, consts, n_consts, ws, ws_bytes, z, rho, wpath,
                                       key, lg, stats, None)


def test_hais_size_query(hip_lib):
    q = hip_lib.cmcd_segment_hais_workspace_bytes
    rec = lambda tiles: (tiles * 10 + 3) // 4 * 16      # one 5-double record per 16-particle tile, rounded up to 16 bytes
    assert q(GMM, 2, 8, 1, 1) == rec(1) == 48 and q(GMM, 2, 8, 3, 17) == rec(2) == 80 and q(MANY, 2, 256, 1, 2000) == rec(125)
    assert q(FUNNEL, 10, 64, 2, 300) == rec(19) == hip_lib.cmcd_reverse_hais_workspace_bytes(FUNNEL, 10, 64, 2, 300)
    assert q(GMM, 2, 4096, 4096, 16) > 0                                    # nbridges * lfsteps = 2^24: the limit itself
    for args, text in (((GMM, 2, 0, 1, 32), "nbridges and lfsteps"), ((GMM, 2, -1, 1, 32), "nbridges and lfsteps"),
                       ((GMM, 2, 8, 0, 32), "nbridges and lfsteps"), ((GMM, 2, 8, 1, 0), "n or dim"), ((GMM, 2, 8, 1, -5), "n or dim"),
                       ((GMM, 0, 8, 1, 32), "n or dim"), ((LGCP, 1600, 8, 1, 32), "lgcp"), ((GMM, 3, 8, 1, 32), "kernel instance"),
                       ((FUNNEL, 2, 8, 1, 32), "kernel instance"), ((GMM, 2, 4097, 1, 32), "nbridges above 4096"),
                       ((GMM, 2, 4096, 4097, 32), "2^24")):
        assert q(*args) == 0 and text in _lib.last_error(), (args, _lib.last_error())


def test_hais_refusals_are_decided_before_any_gpu_work(hip_lib):
    flat, lay = hais_setup()                              # K = 8
    need = hip_lib.cmcd_segment_hais_workspace_bytes(GMM, 2, 8, 1, 32)
    cases = [(dict(**{k: None}), -1, "null pointer") for k in ("params", "ws", "z", "rho", "wpath", "key", "lg", "stats")] + [
        (dict(rho=None, k0=1), -1, "null pointer"),
        (dict(layout=False), -1, "null pointer"),
        (dict(k0=-1), -1, RANGE), (dict(k0=2, k1=2), -1, RANGE), (dict(k0=3, k1=2), -1, RANGE), (dict(k1=9), -1, RANGE),
        (dict(k0=8, k1=9), -1, RANGE),
        (dict(seeds=None), -1, "needs seeds"),
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
    assert hais_call(hip_lib, flat, lay, k0=1, k1=2, seeds=None, ws_bytes=need - 1) == -3      # no seeds needed past bridge 0
    assert hais_call(hip_lib, flat, lay, k0=7, k1=8, L=3, ws_bytes=need - 1) == -3
    with pytest.raises(NotImplementedError, match="lgcp"):
        _lib.check(hais_call(hip_lib, flat, lay, target=LGCP, dim=1600))
    with pytest.raises(ValueError):
        _lib.check(hais_call(hip_lib, flat, lay, k1=9))
    big = _lib.HaisLayout(**{k: getattr(lay, k) for k in _lib.HAIS_LAYOUT_FIELDS})
    big.ngrid = 2000
    assert hais_call(hip_lib, flat, big) == -1 and "ngrid out of range" in _lib.last_error()


# ------------------------------------------------------------------------------------------ the older entry points, the Python layer
def test_the_older_segment_entry_points_keep_refusing_these_modes(hip_lib):
    """cmcd_bound_segment has no momentum; cmcd_bound_segment_uha is the 2nd-order chain (two network evaluations per bridge, the cos^2
    table, the clip).  The descriptor LDVI hands the library carries MCD_CAIS_UHA_sn's value as a placeholder, which cmcd_bound_segment
    refuses; and the Python modules refuse the mode strings, each naming the module that runs them."""
    from cmcd_amd import smc, smc_hais, smc_ldvi, smc_uha
    from cmcd_amd.model_handler import load_model
    flat, desc, lay, use_net = ldvi_setup()
    assert hip_lib.cmcd_segment_workspace_bytes(C.byref(desc), 32) == 0 and "overdamped modes only" in _lib.last_error()
    tgt = load_model("gmm")[0]
    seeds = torch.arange(1, 33, dtype=torch.int32)
    for mode in ("MCD_U_a-lp-sn", "MCD_U_a-lp"):
        f, un, fixed = ldvi.initialize(2, nbridges=8, eps=0.01, emb_dim=20, mode=mode, nn_arch="geffner", device="cpu")
        for mod in (smc, smc_uha):
            with pytest.raises(NotImplementedError):
                mod.segment(seeds, 0, 2, f, un, fixed, tgt)
        with pytest.raises(NotImplementedError, match="cmcd_amd.smc_ldvi"):
            smc_hais.segment(seeds, 0, 2, f, un, fixed, tgt)
        with pytest.raises(NotImplementedError, match="cmcd_amd.smc_ldvi"):
            smc_hais.smc_bound(seeds, f, un, fixed, tgt)
    fh, uh, xh = hais.initialize(dim=2, nbridges=8, lfsteps=1, eps=0.05, eta=0.5, device="cpu")
    with pytest.raises(NotImplementedError, match="cmcd_amd.smc_hais"):
        smc_ldvi.segment(seeds, 0, 2, fh, uh, xh, tgt)
    with pytest.raises(NotImplementedError, match="cmcd_amd.smc_hais"):
        smc_ldvi.smc_bound(seeds, fh, uh, xh, tgt)
    from cmcd_amd import synthetic
    for mode, where in (("MCD_CAIS_sn", r"cmcd_amd\.smc\)"), ("MCD_CAIS_UHA_sn", "cmcd_amd.smc_uha")):
        b = synthetic.build("gmm_n300_k8", device="cpu", boundmode=mode)
        for mod in (smc_ldvi, smc_hais):
            with pytest.raises(NotImplementedError, match=where):
                mod.segment(seeds, 0, 2, b["params_flat"], b["unflatten"], b["params_fixed"], b["target"])


def test_python_entry_points_refuse_host_tensors_and_states_without_momentum(hip_lib):
    from cmcd_amd import smc, smc_hais, smc_ldvi, smc_uha
    from cmcd_amd.model_handler import load_model
    tgt = load_model("gmm")[0]
    seeds = torch.arange(1, 33, dtype=torch.int32)
    state = {"z": torch.zeros(32, 2), "rho": torch.zeros(32, 2), "wpath": torch.zeros(32), "key": torch.zeros(32, 2, dtype=torch.int32)}
    f, un, fixed = ldvi.initialize(2, nbridges=8, eps=0.01, emb_dim=20, mode="MCD_U_a-lp-sn", nn_arch="geffner", device="cpu")
    fh, uh, xh = hais.initialize(dim=2, nbridges=8, lfsteps=1, eps=0.05, eta=0.5, device="cpu")
    for mod, args in ((smc_ldvi, (f, un, fixed, tgt)), (smc_hais, (fh, uh, xh, tgt))):
        assert mod.__all__ == ["STATE_FIELDS", "segment", "losses_of", "resample_stage", "default_cuts", "smc_bound"]
        assert mod.STATE_FIELDS == ("z", "rho", "wpath", "lg", "key") and mod.losses_of is smc.losses_of
        assert mod.resample_stage is smc_uha.resample_stage and mod.default_cuts(8) == [1, 2, 3, 4, 5, 6, 7]      # imported, not copied
        with pytest.raises(RuntimeError, match="runs on a ROCm device only"):
            mod.segment(seeds, 0, 2, *args)
        with pytest.raises(RuntimeError, match="runs on a ROCm device only"):
            mod.segment(state, 2, 4, *args)
        with pytest.raises(TypeError, match="rho"):
            mod.segment({k: v for k, v in state.items() if k != "rho"}, 2, 4, *args)
        with pytest.raises(RuntimeError, match="runs on a ROCm device only"):
            mod.smc_bound(seeds, *args, groups=2)
        with pytest.raises(ValueError, match="cuts"):
            mod.smc_bound(seeds, *args, cuts=[3, 3])
    with pytest.raises(ValueError, match="nbridges"):
        smc_hais.segment(seeds, 0, 1, fh, uh, (2, 0, 1), tgt)
