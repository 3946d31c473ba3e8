"""Captured and side-stream calls: one protocol (`replay_protocol`) and one case table (`CASES`), shared by
tests/test_gpu_capture.py (which runs the protocol on the GPU) and tests/test_capture_cases.py (which asserts on the CPU that the
table is what it says).

Why: a call captured into a graph replays its launches as graph nodes, and every zeroing the library does with hipMemsetAsync
becomes a memset node.  LDVI's gradient call returned garbage from the second replay on, when it ran behind other work of its
stream without a host synchronisation (CHANGELOG.md, round 24); opt.run(use_graph=True) replays the gradient calls below under
exactly that condition.  The eager calls are pinned to float64 autograd case by case and to repeat in the same bits, so
"side stream == eager" and "replay == eager", bit for bit, carry the float64 pin over without a tolerance to choose — provided
the cases are the parity lists' own.  Hence the table: every entry names the parity list it comes from and the key of its entry
there, and is built by that list's own builder (synthetic.build on the list's overrides, gated_cases.build_case,
mfvi_cases.build, lgcp_grad_cases.build).

A case is `(id, family, builder)`; the families are the test functions of tests/test_gpu_capture.py.  Which zeroing site each
case reaches is the table of DESIGN.md section 2, "Captured and side-stream calls".
"""
import numpy as np
import torch

NAMES = ("grad", "losses", "z", "stats")


# ------------------------------------------------------------------------------------------ the protocol
def _leaves_of(unflatten, offsets):
    """Leaf names (with counts) the flat offsets fall in, from unflatten.layout."""
    spans = sorted((off, max(1, int(np.prod(shape))), "/".join(map(str, path))) for path, (off, shape) in unflatten.layout.items())
    starts = np.array([s[0] for s in spans])
    idx = np.searchsorted(starts, np.asarray(offsets), side="right") - 1
    names, counts = np.unique(idx, return_counts=True)
    return {spans[i][2]: int(c) for i, c in zip(names, counts)}


def mismatches(got, want, names, unflatten=None, nonfinite=False):
    """-> one line per tensor of `got` that differs from `want` in bits: how many entries differ, the first indices, the values
    on both sides, and for a gradient the leaves the differing offsets fall in.  `nonfinite`: the gradient is compared after
    nan_to_num (NaN != NaN), everything else as it is."""
    bad = []
    for name, a, b in zip(names, got, want):
        if nonfinite and name == "grad":
            a, b = torch.nan_to_num(a), torch.nan_to_num(b)
        if torch.equal(a, b):
            continue
        if a.shape != b.shape:
            bad.append("%s: shape %s against %s" % (name, tuple(a.shape), tuple(b.shape)))
            continue
        off = torch.nonzero((a != b).flatten()).flatten()
        line = "%s: %d of %d entries differ, first at %s: %s against %s" % (
            name, off.numel(), a.numel(), off[:8].tolist(), a.flatten()[off[:4]].tolist(), b.flatten()[off[:4]].tolist())
        if name == "grad" and unflatten is not None and off.numel():
            line += ", in leaves %s" % _leaves_of(unflatten, off.cpu().numpy())
        bad.append(line)
    return bad


def assert_same_bits(got, want, names, tag, unflatten=None, nonfinite=False):
    bad = mismatches(got, want, names, unflatten, nonfinite)
    assert not bad, (tag, bad)


def _clones(out):
    return [t.clone() for t in out]


def _nan_fill(out):
    """An entry the call never writes must show: NaN, not zero (a gradient is documented as fully overwritten)."""
    for t in out:
        if t.is_floating_point():
            t.fill_(float("nan"))


def replay_protocol(call, params, tag, names=None, unflatten=None, nonfinite=False):
    """`call()` -> a tuple of device tensors (`names`: ("grad", "losses", "z"[, "stats"]) by default; the first one leads: it is
    the one held against a second eager call and the one that must move with the parameters).  `params`: the static params_flat
    `call` reads — a clone, it is updated in place below.  `nonfinite`: the case's eager gradient holds non-finite entries (it is
    asserted which).  Steps: eager; side stream; warm-up and capture on the side stream; three replays into NaN-filled outputs;
    two replays back to back behind other work with no host synchronisation in between; a replay after an in-place parameter
    update.  Every comparison is torch.equal."""
    cur = torch.cuda.current_stream()
    # 1. eager, on the current stream
    eager = _clones(call())
    torch.cuda.synchronize()
    names = NAMES[:len(eager)] if names is None else names
    assert len(names) == len(eager)
    same = lambda got, want, what: assert_same_bits(got, want, names, "%s: %s" % (tag, what), unflatten, nonfinite)
    if names[0] == "grad":
        assert bool(torch.isfinite(eager[0]).all()) != nonfinite, (tag, "the eager gradient is %sfinite" % ("" if nonfinite else "not "))
    # 2. a side stream
    side = torch.cuda.Stream()
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        out = call()
    side.synchronize()
    same(out, eager, "side stream")
    again = _clones(call())
    torch.cuda.synchronize()
    same(out[:1], again[:1], "side stream against a second eager call")
    del out, again
    # 3. warm-up on the capture stream, capture
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        call()
    cur.wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        captured = call()
    # 4. three replays, each into NaN-filled outputs
    for rep in range(3):
        _nan_fill(captured)
        graph.replay()
        torch.cuda.synchronize()
        same(captured, eager, "replay %d" % rep)
    # 5. back to back: the second replay follows the first, the clones, the fill and an unrelated launch with no host
    # synchronisation in between
    noise = torch.randn(1 << 20, device=params.device)
    torch.cuda.synchronize()
    graph.replay()
    first = _clones(captured)
    _nan_fill(captured)
    noise = noise * 1.0001
    graph.replay()
    second = _clones(captured)
    torch.cuda.synchronize()
    same(first, eager, "back-to-back replay 0")
    same(second, eager, "back-to-back replay 1")
    # 6. the graph reads the parameters it was captured on, in place
    params.mul_(1.001)
    _nan_fill(captured)
    graph.replay()
    torch.cuda.synchronize()
    updated = _clones(call())
    torch.cuda.synchronize()
    same(captured, updated, "replay after an in-place parameter update")
    # ... and they matter: the gradient moves (a call without one: some output does — a mean may be +inf before and after)
    moved = [not torch.equal(torch.nan_to_num(a), torch.nan_to_num(b)) for a, b in zip(updated, eager)]
    assert moved[0] if names[0] == "grad" else any(moved), (tag, "the call ignores its parameters")


# ------------------------------------------------------------------------------------------ builders
class Builder:
    """Where a case comes from and how it is called.  `source`: the parity list; `key`: the entry's index or id there; `expect`:
    what that entry must be ((config, n, overrides) of a list entry, compared whole; unused for the id-keyed lists), so that a list that is reordered fails
    the CPU test instead of silently swapping the case.  `resolve()` needs no GPU; `build(monkeypatch)` ->
    dict(call, params, unflatten, names, nonfinite)."""
    source = None

    def __init__(self, key, expect=None, item=None, variant=None, entry=None):
        self.key, self.expect, self.item, self.variant, self.entry = key, expect, item, variant, entry

    def _pin(self, monkeypatch):
        """The parity tests' own switches: the dense parameter set, the gradient path, the forward's kernel form."""
        from cmcd_amd import mcdboundingmachine as mcdbm
        from cmcd_amd import synthetic
        monkeypatch.setattr(synthetic, "DENSE_DEFAULT", True)
        if self.item is not None:
            monkeypatch.setenv("CMCD_GRAD_ITEM", str(self.item))
        if self.variant is not None:
            monkeypatch.setattr(mcdbm, "KERNEL_VARIANT", self.variant)


def _mcd_call(fn_name, seeds, params, b, kw):
    """compute_log_var_grad -> (grad, losses, z); compute_bound_grad -> (grad, losses, z, stats)."""
    from cmcd_amd import mcdboundingmachine as mcdbm
    fn = getattr(mcdbm, fn_name)
    args = (seeds, params, b["unflatten"], b["params_fixed"], b["target"])
    if fn_name == "compute_log_var_grad":
        def call():
            grad, (losses, z) = fn(*args, **kw)
            return grad, losses, z
    else:
        def call():
            grad, (losses, z), stats = fn(*args, return_stats=True, **kw)
            return grad, losses, z, stats
    return call


class ListCase(Builder):
    """An entry `(config, n, overrides)` of CASES / BPTT_CASES / ULA_CASES (tests/test_gpu_grad.py) or GRAD_CASES
    (tests/test_gpu_uha.py), built and called as the list's parity test does.  `entry`: the boundmode the parity test adds
    (MCD_ULA_sn / MCD_ULA on ULA_CASES, MCD_CAIS_UHA_sn on GRAD_CASES)."""
    MODULE = {"CASES": "test_gpu_grad", "BPTT_CASES": "test_gpu_grad", "ULA_CASES": "test_gpu_grad", "GRAD_CASES": "test_gpu_uha"}

    def __init__(self, source, key, expect, **kw):
        super().__init__(key, expect, **kw)
        self.source = source

    def resolve(self):
        cases = getattr(__import__(self.MODULE[self.source]), self.source)
        name, n, over = cases[self.key]
        assert (name, n, over) == tuple(self.expect), (self.source, self.key, cases[self.key], self.expect)
        return cases[self.key]

    def build(self, monkeypatch):
        from cmcd_amd import synthetic
        self._pin(monkeypatch)
        name, n, over = self.resolve()
        over = dict(over, boundmode=self.entry) if self.entry else over
        b = synthetic.build(name, device="cuda", **over)
        mode = b["params_fixed"][2]
        assert mode == {"CASES": "MCD_CAIS_var_sn", "BPTT_CASES": "MCD_CAIS_sn"}.get(self.source, self.entry)
        seeds = torch.from_numpy(synthetic.parity_seeds(n)).cuda()
        params = b["params_flat"].clone()
        # test_ula_gradient_matches_autograd passes neither a schedule nor the clip flag
        kw = {} if mode == "MCD_ULA" else dict(eps_schedule=b["eps_schedule"], grad_clipping=b["grad_clipping"])
        fn = "compute_log_var_grad" if mode == "MCD_CAIS_var_sn" else "compute_bound_grad"
        return dict(call=_mcd_call(fn, seeds, params, b, kw), params=params, unflatten=b["unflatten"], names=None, nonfinite=False)


class GatedCase(Builder):
    """A case of tests/gated_cases.py by id (gc.case_by_id), built by gc.build_case and called as test_gpu_grad.gated_call does."""
    source = "gc.case_by_id"

    def resolve(self):
        import gated_cases as gc
        return gc.case_by_id(self.key)

    def build(self, monkeypatch):
        import gated_cases as gc
        self._pin(monkeypatch)
        case = self.resolve()
        b = gc.build_case(case, device="cuda")
        seeds = torch.from_numpy(np.asarray(case[3], np.int32)).cuda()
        params = b["params_flat"].clone()
        fn = "compute_log_var_grad" if case[4] == "MCD_CAIS_var_sn" else "compute_bound_grad"
        kw = dict(eps_schedule=b["eps_schedule"], grad_clipping=b["grad_clipping"])
        # floored particles and clamped outputs leave the gradient finite (test_gradient_paths_agree_where_a_gate_acts)
        return dict(call=_mcd_call(fn, seeds, params, b, kw), params=params, unflatten=b["unflatten"], names=None, nonfinite=False)


class MfviCase(Builder):
    """A case of tests/mfvi_cases.py by id; entry "grad": boundingmachine.grad_and_loss -> (grad, losses, z), "bound":
    boundingmachine.compute_bound -> (mean, losses, z)."""
    source = "mc.case_by_id"

    def resolve(self):
        import mfvi_cases as mc
        return mc.case_by_id(self.key)

    def build(self, monkeypatch):
        import mfvi_cases as mc
        from cmcd_amd import boundingmachine as bm
        case = self.resolve()
        target, _, dim, flat, unflatten, fixed, _ = mc.build(case, "cuda")[:7]
        seeds = torch.from_numpy(np.ascontiguousarray(mc.seeds_of(case), np.int32)).cuda()
        params = flat.clone()
        fn = bm.grad_and_loss if self.entry == "grad" else bm.compute_bound

        def call():
            lead, (losses, z) = fn(seeds, params, unflatten, fixed, target)
            return lead, losses, z
        names = ("grad", "losses", "z") if self.entry == "grad" else ("mean", "losses", "z")
        return dict(call=call, params=params, unflatten=unflatten, names=names, nonfinite=False)


class LgcpCase(Builder):
    """A case of tests/lgcp_grad_cases.py by id on the dense parameter set, KERNEL_VARIANT = the case's form; entry "grad": lc.call
    (with the statistics where the entry point returns them), "forward": lc.forward -> (losses, z, stats)."""
    source = "lc.case_by_id"

    def resolve(self):
        import lgcp_grad_cases as lc
        return lc.case_by_id(self.key)

    def facts(self):
        return lgcp_facts(self.resolve(), forward_only=self.entry == "forward")

    def build(self, monkeypatch):
        import lgcp_grad_cases as lc
        from cmcd_amd import mcdboundingmachine as mcdbm
        case = self.resolve()
        monkeypatch.setattr(mcdbm, "KERNEL_VARIANT", case[4])
        b = dict(lc.build(case, "dense"))
        params = b["params_flat"] = b["params_flat"].clone()
        seeds = torch.from_numpy(np.ascontiguousarray(lc.seeds_of(case))).cuda()
        if self.entry == "forward":
            return dict(call=lambda: lc.forward(b, seeds), params=params, unflatten=b["unflatten"],
                        names=("losses", "z", "stats"), nonfinite=False)
        if case[1] == lc.VAR:
            def call():
                grad, (losses, z) = lc.call(b, seeds)
                return grad, losses, z
        else:
            def call():
                grad, (losses, z), stats = lc.call(b, seeds, return_stats=True)
                return grad, losses, z, stats
        return dict(call=call, params=params, unflatten=b["unflatten"], names=None, nonfinite=False)


class LgcpWideCase(Builder):
    """The wide-batch forward in the configuration of test_gpu_fullsize.test_lgcp_prepared_tables: key = its (n, k)."""
    source = "test_lgcp_prepared_tables"

    def resolve(self):
        import test_gpu_fullsize as tf
        mark = next(m for m in tf.test_lgcp_prepared_tables.pytestmark if m.name == "parametrize")
        assert mark.args[0] == "n,k"
        return next(nk for nk in mark.args[1] if tuple(nk) == tuple(self.key))

    def facts(self):
        n, _ = self.resolve()
        return dict(passes=None, lanes=1, kept=None, side_streams=False, wide=n >= LGCP_WIDE_MIN)

    def build(self, monkeypatch):
        from cmcd_amd import mcdboundingmachine as mcdbm
        from cmcd_amd import synthetic
        from helpers import lgcp_counts_fixture
        n, k = self.resolve()
        b = synthetic.build("lgcp_n20_k128", device="cuda", lgcp_counts=lgcp_counts_fixture(), nbridges=k, N=n, dense=True)
        seeds = torch.from_numpy(synthetic.throughput_seeds(n, stream=6)).cuda()
        params = b["params_flat"].clone()
        args = (b["unflatten"], b["params_fixed"], b["target"])
        return dict(call=lambda: mcdbm.bound_forward(seeds, params, *args), params=params, unflatten=b["unflatten"],
                    names=("losses", "z", "stats"), nonfinite=False)


# ------------------------------------------------------------------------------------------ the launch rules at d = 1600
# Restated from cmcd_lgcp.hip (lgcp_lanes, lgcp_shape's nsk rule at both widths, lgcp_grad_ws / lgcp_keep, lgcp_uha_grad_ws,
# lgcp_use_wide) and cmcd_common.h, on lc.passes_of: what a case reaches, so that a changed rule fails an assertion instead of
# silently un-testing a site.
LGCP_LANES = 4                  # kLanes
LGCP_NSK_INPUTS = 16 * 104      # 16 * kNskChunks
LGCP_KEEP_FLOATS = 1 << 28      # the kept tables' cap
LGCP_WIDE_MIN = 225             # kLgcpWideMin


def lgcp_facts(case, forward_only=False):
    """-> dict(passes, lanes, kept, side_streams, wide) of a case of tests/lgcp_grad_cases.py.
      passes        lc.passes_of(n);
      lanes         passes the forward runs side by side, lane 0 on the caller's stream and the others on side streams
                    (lgcp_lanes); the 2nd-order sequence walks its passes in turn on the caller's stream: 1;
      kept          the forward keeps every evaluation's activations for the reverse sweep (lgcp_keep); False:
                    the sweep recomputes them — overdamped: on a side stream; None for a forward-only call;
      side_streams  the call forks work onto another stream, i.e. its captured graph has parallel branches;
      wide          a forward-only call of >= 225 particles takes the wide-batch path (one stream)."""
    import lgcp_grad_cases as lc
    _, mode, n, K, form, over = case
    D, emb = lc.D, over.get("emb_dim", 20)
    uha = mode == lc.UHA
    passes = lc.passes_of(n)
    wide = forward_only and not uha and form == 0 and n >= LGCP_WIDE_MIN and D % 4 == 0 and (D + emb) % 4 == 0
    lanes = 1 if (uha or wide) else min(len(passes), LGCP_LANES)
    if forward_only:
        return dict(passes=passes, lanes=lanes, kept=None, side_streams=lanes > 1, wide=wide)
    if uha:
        IN, R = 2 * D + emb, 2 * K * n
        nsk = form != 3 and D % 16 == 0 and D <= LGCP_NSK_INPUTS and IN <= 2 * LGCP_NSK_INPUTS
        kept = nsk and R * (2 * IN + D) + (K + 1) * n * D <= LGCP_KEEP_FLOATS
        return dict(passes=passes, lanes=1, kept=kept, side_streams=False, wide=False)
    IN, R = D + emb, (K + 1) * n
    nsk = form != 3 and D % 16 == 0 and IN <= LGCP_NSK_INPUTS
    kept = nsk and R * (2 * IN + 2 * D) <= LGCP_KEEP_FLOATS
    return dict(passes=passes, lanes=lanes, kept=kept, side_streams=lanes > 1 or not kept, wide=False)


def _facts(passes, lanes, kept, side_streams, wide=False):
    return dict(passes=passes, lanes=lanes, kept=kept, side_streams=side_streams, wide=wide)


# what each d = 1600 case is in the table for (asserted against lgcp_facts on the CPU and before the GPU run)
LGCP_FACTS = {
    "lgcp-n20": _facts([20], 1, True, False),             # one pass, kept activations, the no-split-K products
    "lgcp-n21": _facts([21], 1, True, False),             # split-K products on kept activations
    "lgcp-var-n21": _facts([21], 1, True, False),
    "lgcp-ulasn-n17": _facts([17], 1, True, False),
    "lgcp-ula-n20": _facts([20], 1, True, False),
    "lgcp-uha-n17": _facts([17], 1, True, False),
    "lgcp-fwd-n20": _facts([20], 1, None, False),
    "lgcp-n33": _facts([32, 1], 2, True, True),           # the forward forks a lane; the `base > 0` clears of lgcp_grad run
    "lgcp-rc-n21": _facts([21], 1, False, True),          # form 3: the sweep's two-stream recompute
    "lgcp-uha-n33": _facts([32, 1], 1, True, False),      # two passes in turn on one stream: lgcp_uha_grad's `base > 0` clear
    # form 3 of the 2nd-order mode: the split-K forward (its counter clear) and the recompute sweep (its lgcp_zero launches), two
    # passes in turn on one stream
    "lgcp-uha-rc-n33": _facts([32, 1], 1, False, False),
    "lgcp-fwd-n33": _facts([32, 1], 2, None, True),
    "lgcp-wide-n230": _facts(None, 1, None, False, wide=True),
}

_GMM, _FUNNEL, _MANY_VAR, _MANY_DDS = "gmm_n300_k8", "funnel_n300_k64", "many_gmm_var_n16000_k256", "many_gmm_n2000_k256_dds"
_VAR = [("gmm", 2, (_GMM, 128, dict(boundmode="MCD_CAIS_var_sn", grad_clipping=True))),
        ("funnel-dds", 5, (_FUNNEL, 40, dict(boundmode="MCD_CAIS_var_sn", nbridges=5, nn_arch="dds"))),
        ("many132", 7, (_MANY_VAR, 80, dict(nbridges=5)))]
_BPTT = [("gmm", 3, (_GMM, 128, {})), ("funnel", 5, (_FUNNEL, 70, dict(nbridges=6)))]
_ULA0 = (_MANY_DDS, 70, dict(nbridges=6, init_sigma=15.0, init_eps=0.2))
_UHA = [("gmm", 0, (_GMM, 128, {})), ("funnel", 4, (_FUNNEL, 70, dict(nbridges=6, init_eps=0.05, init_gamma=4.0)))]

CASES = (
    # ---- tests/test_gpu_grad.py: VarGrad on both item paths (item 0: the two memsets of grad_launch)
    [("var-%s-item%d" % (tag, item), "mcd", ListCase("CASES", key, expect, item=item)) for tag, key, expect in _VAR for item in (0, 1)]
    # ---- the reparameterised gradient: item 0 = memsets, item 1 = the Jacobian launch zeroes; forward variant 1, gmm also on 3
    + [("bptt-%s-v1-item%d" % (tag, item), "mcd", ListCase("BPTT_CASES", key, expect, item=item, variant=1))
       for tag, key, expect in _BPTT for item in (0, 1)]
    + [("bptt-gmm-v3-item1", "mcd", ListCase("BPTT_CASES", 3, (_GMM, 128, {}), item=1, variant=3))]
    # ---- the overdamped baselines: grad_launch with ula = 2, and ula_grad_launch
    + [("ulasn-many", "mcd", ListCase("ULA_CASES", 0, _ULA0, item=0, variant=1, entry="MCD_ULA_sn")),
       ("ula-many", "mcd", ListCase("ULA_CASES", 0, _ULA0, entry="MCD_ULA"))]
    # ---- floored particles and clamped outputs (both in test_gpu_grad.REPEAT_CASES)
    + [("gated-floor-mid-item0", "mcd", GatedCase("floor-mid", item=0)),
       ("gated-clamp-dds-gmm-item1", "mcd", GatedCase("clamp-dds-gmm", item=1))]
    # ---- tests/test_gpu_uha.py: 2nd-order, whole chains (the memsets of uha_grad_launch) and work items
    + [("uha-%s-item%d" % (tag, item), "uha", ListCase("GRAD_CASES", key, expect, item=item, entry="MCD_CAIS_UHA_sn"))
       for tag, key, expect in _UHA for item in (0, 1)]
    + [("uha-gated-floor-item%d" % item, "uha", GatedCase("uha-floor", item=item)) for item in (0, 1)]
    # ---- tests/mfvi_cases.py
    + [("mfvi-%s-%s" % (cid, entry), "mfvi", MfviCase(cid, entry=entry))
       for cid in ("gmm-145", "funnel-21", "floor-half", "lgcp-33") for entry in ("grad", "bound")]
    # ---- tests/lgcp_grad_cases.py, the call on the caller's stream alone
    + [("lgcp-" + cid, "lgcp_one_stream", LgcpCase(cid, entry="grad")) for cid in ("n20", "n21", "var-n21", "ulasn-n17", "ula-n20", "uha-n17")]
    + [("lgcp-fwd-n20", "lgcp_one_stream", LgcpCase("n20", entry="forward"))]
    # ---- d = 1600 with side streams (uha-n33 and uha-rc-n33 sit here with their pass count; their sequences stay on one stream)
    + [("lgcp-" + cid, "lgcp_forked_streams", LgcpCase(cid, entry="grad")) for cid in ("n33", "rc-n21", "uha-n33", "uha-rc-n33")]
    + [("lgcp-fwd-n33", "lgcp_forked_streams", LgcpCase("n33", entry="forward")),
       ("lgcp-wide-n230", "lgcp_forked_streams", LgcpWideCase((230, 2)))]
)
FAMILIES = ("mcd", "uha", "mfvi", "lgcp_one_stream", "lgcp_forked_streams")


def cases_of(family):
    return [c for c in CASES if c[1] == family]


def ids_of(family):
    return [c[0] for c in cases_of(family)]


def case_by_id(cid):
    return next(c for c in CASES if c[0] == cid)


def run_case(cid, monkeypatch):
    """Builds the case and runs the protocol on it; a d = 1600 case first asserts what it is there for."""
    _, _, builder = case_by_id(cid)
    if cid in LGCP_FACTS:
        assert builder.facts() == LGCP_FACTS[cid], (cid, builder.facts())
    built = builder.build(monkeypatch)
    replay_protocol(built["call"], built["params"], cid, names=built["names"], unflatten=built["unflatten"],
                    nonfinite=built["nonfinite"])
