"""cmcd_amd._chain alone, without a GPU: the state checks of the four segment families with their exception types and texts, the
driver loop's refusals, the size-query cache's rule, the call path itself on CPU tensors with a fake C call, and the two
functions that pick a module by boundmode.  The device checks of `_call` are stepped over where a test says so."""
import pytest
import torch

from cmcd_amd import _chain, hais, ldvi, smc, smc_hais, smc_ldvi, smc_uha, synthetic
from cmcd_amd import mcdboundingmachine as mcdbm
from cmcd_amd import reverse_hais, reverse_ldvi, reverse_uha
from cmcd_amd.model_handler import load_model

N, DIM, K = 32, 2, 8
MISSING = {
    smc: "a segment with k0 > 0 starts from the state dict an earlier segment (or resample_stage) returned",
    smc_uha: "a 2nd-order segment with k0 > 0 starts from the state dict an earlier smc_uha.segment (or resample_stage) returned: "
             "z, rho, wpath and key",
    smc_ldvi: "an LDVI segment with k0 > 0 starts from the state dict an earlier smc_ldvi.segment (or resample_stage) returned: "
              "z, rho, wpath and key",
    smc_hais: "a UHA segment with k0 > 0 starts from the state dict an earlier smc_hais.segment (or resample_stage) returned: "
              "z, rho, wpath and key",
}


def _args(mod):
    """(params_flat, unflatten, params_fixed, target) of the module's family, on the CPU."""
    tgt = load_model("gmm")[0]
    if mod is smc_ldvi:
        return (*ldvi.initialize(DIM, nbridges=K, eps=0.01, emb_dim=20, mode="MCD_U_a-lp-sn", nn_arch="geffner", device="cpu"), tgt)
    if mod is smc_hais:
        return (*hais.initialize(dim=DIM, nbridges=K, lfsteps=1, eps=0.05, eta=0.5, device="cpu"), tgt)
    b = synthetic.build("gmm_n300_k8", device="cpu", **({"boundmode": "MCD_CAIS_UHA_sn"} if mod is smc_uha else {}))
    return b["params_flat"], b["unflatten"], b["params_fixed"], b["target"]


def _state(mod):
    st = {"z": torch.zeros(N, DIM), "wpath": torch.zeros(N), "key": torch.zeros(N, 2, dtype=torch.int32)}
    if mod is not smc:
        st["rho"] = torch.zeros(N, DIM)
    return st


@pytest.fixture
def on_host(monkeypatch):
    """Steps over the device checks: params_flat may be a host tensor, the call runs on 'device 0, stream 0' and takes its
    workspace from the host.  -> the list of (nbytes, tag, what, retire) the workspace was asked for."""
    asked = []

    def inputs(seeds, params_flat, seedless=False):
        return (None, 0) if seedless else (torch.as_tensor(seeds, dtype=torch.int32), len(seeds))

    def workspace(dev_index, device, stream, capturing, nbytes, tag, what=None, retire=False):
        asked.append((nbytes, tag, what, retire))
        if nbytes <= 0:
            raise NotImplementedError(what)
        return torch.empty(nbytes, dtype=torch.uint8)

    monkeypatch.setattr(_chain, "_inputs", inputs)
    monkeypatch.setattr(_chain, "_workspace", workspace)
    monkeypatch.setattr(_chain, "on_device", lambda device, body: body(0, 0, False))
    return asked


@pytest.mark.parametrize("mod", [smc, smc_uha, smc_ldvi, smc_hais], ids=lambda m: m.__name__.rsplit(".", 1)[1])
def test_state_checks_keep_their_exception_types_and_texts(mod, on_host):
    args = _args(mod)
    good = _state(mod)
    mats = "z" if mod is smc else "z and rho"
    floats = "z and wpath" if mod is smc else "z, rho and wpath"
    for bad in (None, 7, [good], {k: v for k, v in good.items() if k != "key"}, {k: v for k, v in good.items() if k != "z"}):
        with pytest.raises(TypeError) as e:
            mod.segment(bad, 2, 4, *args)
        assert str(e.value) == MISSING[mod]
    if mod is not smc:
        with pytest.raises(TypeError) as e:
            mod.segment({k: v for k, v in good.items() if k != "rho"}, 2, 4, *args)
        assert str(e.value) == MISSING[mod]
    for field, value in (("z", good["z"].double()), ("wpath", good["wpath"].half()), ("key", good["key"].long()),
                         ("wpath", torch.zeros(0))) + ((("rho", good["rho"].double()),) if mod is not smc else ()):
        with pytest.raises(ValueError) as e:
            mod.segment(dict(good, **{field: value}), 2, 4, *args)
        assert str(e.value) == f"state: {floats} must be float32, key int32"
    for field, value in (("z", torch.zeros(N, 3)), ("z", torch.zeros(N + 1, DIM)), ("key", torch.zeros(N, 3, dtype=torch.int32)),
                         ("key", torch.zeros(N, dtype=torch.int32))) + ((("rho", torch.zeros(N, 3)),) if mod is not smc else ()):
        with pytest.raises(ValueError) as e:
            mod.segment(dict(good, **{field: value}), 2, 4, *args)
        assert str(e.value) == f"state: {mats} must have shape [{N}, {DIM}] and key [{N}, 2]"
    for field in good:
        with pytest.raises(RuntimeError) as e:
            mod.segment(dict(good, **{field: good[field].numpy()}), 2, 4, *args)
        assert str(e.value) == (f"the CMCD hot path runs on a ROCm device only: state[{field!r}] is not a tensor on the device of "
                                "params_flat")


def test_the_overdamped_segment_checks_params_flat_before_the_state_and_the_others_after_it():
    """Without the fixture: params_flat is a host tensor, which `_call._inputs` refuses."""
    for mod in (smc, smc_uha, smc_ldvi, smc_hais):
        args = _args(mod)
        with pytest.raises(RuntimeError if mod is smc else TypeError):
            mod.segment(None, 2, 4, *args)
        with pytest.raises(RuntimeError, match="params_flat is not a device tensor"):
            mod.segment(_state(mod), 2, 4, *args)


class _Consts:
    """A target whose constants are a 3-float tensor."""
    t = torch.zeros(3)

    def consts_on(self, device):
        return self.t


@pytest.mark.parametrize("momentum", [False, True], ids=["overdamped", "momentum"])
@pytest.mark.parametrize("k0", [0, 3])
def test_segment_call_hands_fresh_tensors_to_the_c_call_and_returns_the_state(momentum, k0, on_host):
    fields = ("z", "rho", "wpath", "key") if momentum else ("z", "wpath", "key")
    state = {"z": torch.ones(N, DIM), "rho": torch.ones(N, DIM).t().contiguous().t(), "wpath": torch.ones(N, 1),
             "key": torch.ones(N, 2, dtype=torch.int32), "lg": torch.ones(N), "stats": None, "k": 3}
    params, tgt, seen, asked = torch.zeros(4), _Consts(), [], []

    def query(a, b, n):
        asked.append((a, b, n))
        return 640 + n

    def fn(*args):
        seen.append(args)
        return 0

    shape = ("test_chain_call", object())      # a key no other test has put into the cache
    run = lambda st, q=query, f=fn, hint=None: _chain.segment_call(
        st, k0, 6, params, DIM, momentum, "no state", "tag", "no kernel", True, q, ("qa", "qb"), shape, f, ("h0", "h1", k0, 6),
        tgt.consts_on, hint=hint)
    got = run(list(range(1, N + 1)) if k0 == 0 else state)
    assert list(got) == [*fields[:-1], "lg", "key", "stats", "k"] and got["k"] == 6
    assert asked == [("qa", "qb", N)] and on_host == [(640 + N, "tag", "no kernel", True)]
    args = seen[0]
    assert args[:4] == ("h0", "h1", k0, 6) and (args[4] is None) == (k0 != 0) and args[5] == N and args[-1] == 0
    assert args[6:10] == (params.data_ptr(), 4, tgt.t.data_ptr(), 3) and args[11] == 640 + N
    assert args[12:-1] == tuple(got[f].data_ptr() for f in (*fields, "lg", "stats"))      # the C call's order: lg behind the key
    assert got["wpath"].shape == (N,) and got["key"].shape == (N, 2) and got["key"].dtype == torch.int32
    assert got["lg"].shape == (N,) and got["stats"].shape == (5,) and got["stats"].dtype == torch.float64
    assert all(got[f].shape == (N, DIM) and got[f].dtype == torch.float32 and got[f].is_contiguous() for f in fields[:-2])
    if k0:      # fresh copies: the state handed in is not what the library overwrites
        assert all(got[f].data_ptr() != state[f].data_ptr() and torch.equal(got[f].reshape(state[f].shape), state[f]) for f in fields)
    run(state if k0 else [1] * N)
    assert len(asked) == 1 and len(seen) == 2      # the size is asked once per (tag, shape, n)
    # a refusing size query (asked every time, with the module's hint behind the library's words) and a failing C call
    for _ in range(2):
        with pytest.raises(NotImplementedError, match="no kernel$"):
            _chain.segment_call(state if k0 else [1], k0, 6, params, DIM, momentum, "no state", "tag", "no kernel", False,
                                lambda n: asked.append(n) or 0, (), ("test_chain_call", "refused"), fn, (), tgt.consts_on)
    assert len(asked) == 3
    from cmcd_amd import _lib
    if not _lib.last_error():
        with pytest.raises(NotImplementedError, match="no kernel: elsewhere$"):
            _chain.segment_call(state if k0 else [1], k0, 6, params, DIM, momentum, "no state", "tag", "no kernel", False,
                                lambda n: -1, (), ("test_chain_call", "refused"), fn, (), tgt.consts_on, hint=": elsewhere")
    with pytest.raises(ValueError):
        run(state if k0 else [1] * N, f=lambda *a: -1)
    if k0:
        with pytest.raises(TypeError, match="no state"):
            run({"z": state["z"]})


def test_reverse_call_with_and_without_momentum(on_host, monkeypatch):
    monkeypatch.setattr(_chain, "check_x", lambda x, n, dim, device: None)
    params, x, tgt = torch.zeros(4), torch.zeros(N, DIM), _Consts()
    for momentum in (False, True):
        seen = []

        def fn(*args):
            seen.append(args)
            return 0

        for head in (("h0", "h1"), lambda: ("h0", "h1")):      # a callable head is resolved in front of the C call
            out = _chain.reverse_call(list(range(N)), x, params, DIM, momentum, "rev", "none", False, lambda a, n: 64, ("qa",),
                                      ("test_chain_call", "reverse", momentum), fn, head, tgt.consts_on)
            assert len(out) == 3 + momentum and out[1].shape == (N, DIM) and out[-1].shape == (5,)
            args = seen[-1]
            assert args[:2] == ("h0", "h1") and args[3:5] == (x.data_ptr(), N) and args[-1] == 0
            assert args[5:9] == (params.data_ptr(), 4, tgt.t.data_ptr(), 3) and args[10] == 64
            assert args[11:-1] == tuple(t.data_ptr() for t in out)
        out[0].fill_(2.0)
        out[-1].fill_(2.0 * N)
        eubo, (w, z0) = _chain.eubo_of(out)
        assert float(eubo) == 2.0 and eubo.dtype == torch.float32 and w is out[0] and z0 is out[1]
    assert mcdbm.eubo_of is _chain.eubo_of
    with pytest.raises(ValueError):
        _chain.reverse_call(list(range(N)), x, params, DIM, True, "rev", "none", False, lambda n: 64, (), "s", lambda *a: -1, (),
                            tgt.consts_on)


def test_size_queries_are_kept_once_answered_and_bounded():
    key = ("test_chain_call", object(), 1)
    assert _chain._ask_size(key, lambda n: 0, (), 1, "what", None) == 0 and key not in _chain._sizes      # a refusal is not kept
    assert _chain._ask_size(key, lambda a, n: a + n, (47,), 1, "what", None) == 48 and _chain._sizes[key] == 48
    for i in range(2 * _chain._SIZE_CACHE):
        _chain._ask_size(("test_chain_call", i, 1), lambda n: 16, (), 1, "what", None)
    assert len(_chain._sizes) <= _chain._SIZE_CACHE and key not in _chain._sizes      # bounded, oldest first


def test_the_driver_refuses_bad_cuts_and_groups(on_host):
    seeds = list(range(1, N + 1))
    for mod in (smc, smc_uha, smc_ldvi, smc_hais):
        args = _args(mod)
        for cuts in ([3, 3], [0, 4], [4, K], [5, 2], [-1]):
            with pytest.raises(ValueError) as e:
                mod.smc_bound(seeds, *args, cuts=cuts)
            assert str(e.value) == f"cuts must be ascending bridges inside (0, {K})"
        for groups in (0, -2, 5, N + 1):
            with pytest.raises(ValueError) as e:
                mod.smc_bound(seeds, *args, groups=groups)
            assert str(e.value) == "N must be a multiple of groups"
    assert _chain.default_cuts(8) == [1, 2, 3, 4, 5, 6, 7] and _chain.default_cuts(64) == list(range(8, 64, 8))
    assert _chain.default_cuts(1) == [] and smc.default_cuts is _chain.default_cuts and smc.losses_of is _chain.losses_of


def test_the_driver_runs_segments_and_stages_in_order(on_host, monkeypatch):
    """The loop on a fake segment: which calls it makes, and "rho" in the result only for a momentum state."""
    for momentum in (False, True):
        log = []

        def segment(state, k0, k1, *args):
            log.append(("segment", k0, k1))
            st = {"z": torch.zeros(N, DIM), "wpath": torch.zeros(N), "lg": torch.zeros(N), "key": None, "stats": None, "k": k1}
            return dict(st, rho=torch.ones(N, DIM)) if momentum else st

        def stage(state, groups, threshold, seed, mom):
            log.append(("stage", state["k"], groups, seed, mom))
            z = torch.zeros(groups, dtype=torch.float64)
            return state, {"resampled": z > 1, "ess": z, "ln_Z_increment": z, "ancestors": None}

        monkeypatch.setattr(_chain, "resample_stage", stage)
        monkeypatch.setattr(_chain.resample, "importance_stats", lambda losses, groups: {"ess": torch.zeros(groups, dtype=torch.float64),
                                                                                         "ln_Z": torch.zeros(groups, dtype=torch.float64)})
        out = _chain.drive(segment, momentum, list(range(N)), torch.zeros(4), None, (DIM, K), None, None, False, 2, [2, 5], 0.5, 10, True)
        assert log == [("segment", 0, 2), ("stage", 2, 2, 12, momentum), ("segment", 2, 5), ("stage", 5, 2, 15, momentum), ("segment", 5, K)]
        assert list(out) == ["ln_Z", "losses", "z"] + (["rho"] if momentum else []) + ["resampled", "ess", "trace"]
        assert out["resampled"].shape == (2, 2) and out["ess"].shape == (3, 2) and [s["k"] for s in out["trace"]] == [2, 5, K]


def test_resample_stage_names_keep_the_missing_momentum_refusal():
    state = dict(_state(smc), lg=torch.zeros(N))
    for mod in (smc_uha, smc_ldvi, smc_hais):
        assert mod.resample_stage is smc_uha.resample_stage
        with pytest.raises(TypeError) as e:
            mod.resample_stage(state)
        assert str(e.value) == "a 2nd-order state carries the momentum: state['rho'] is missing"
    for mod in (smc, smc_uha):
        with pytest.raises(ValueError, match="N must be a multiple of groups"):
            mod.resample_stage(dict(state, rho=torch.zeros(N, DIM)), groups=5)


@pytest.mark.parametrize("boundmode,smc_mod,rev_mod", [
    ("MCD_CAIS_sn", smc, mcdbm), ("MCD_CAIS_var_sn", smc, mcdbm), ("MCD_ULA", smc, mcdbm), ("MCD_ULA_sn", smc, mcdbm),
    ("MCD_CAIS_UHA_sn", smc_uha, reverse_uha), ("MCD_U_a-lp-sn", smc_ldvi, reverse_ldvi), ("MCD_U_a-lp", smc_ldvi, reverse_ldvi),
    ("UHA", smc_hais, reverse_hais)])
def test_modules_by_boundmode_are_the_ones_the_drivers_picked(boundmode, smc_mod, rev_mod):
    assert _chain.smc_module(boundmode) is smc_mod and _chain.reverse_module(boundmode) is rev_mod
