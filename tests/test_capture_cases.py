"""tests/capture_cases.py on the CPU: the table is well-formed, every entry is an entry of the parity list it names, and the
d = 1600 cases reach the passes, lanes and kept / recompute forms they are in the table for."""
import inspect

import capture_cases as cc
import lgcp_grad_cases as lc


def test_the_table_is_well_formed():
    ids = [c[0] for c in cc.CASES]
    assert len(set(ids)) == len(ids)
    for cid, family, builder in cc.CASES:
        assert isinstance(cid, str) and cid and " " not in cid
        assert family in cc.FAMILIES
        assert isinstance(builder, cc.Builder) and builder.source
        assert builder.item in (None, 0, 1) and builder.variant in (None, 1, 2, 3)
    assert all(cc.cases_of(f) for f in cc.FAMILIES)
    assert sum(len(cc.cases_of(f)) for f in cc.FAMILIES) == len(cc.CASES)
    # each family's cases, as the test functions of tests/test_gpu_capture.py take them
    import test_gpu_capture as tg
    fns = [name for name, _ in inspect.getmembers(tg, inspect.isfunction) if name.startswith("test_")]
    assert sorted(fns) == sorted("test_" + ("mcd_gradient" if f == "mcd" else "uha_gradient" if f == "uha" else f) for f in cc.FAMILIES)
    src = inspect.getsource(tg)
    assert src.rindex("\ndef test_") == src.index("\ndef test_lgcp_forked_streams")      # the last function of the file


def test_every_entry_is_an_entry_of_its_parity_list():
    import gated_cases as gc
    import mfvi_cases as mc
    import test_gpu_grad as tgrad
    import test_gpu_uha as tuha
    lists = {"CASES": tgrad.CASES, "BPTT_CASES": tgrad.BPTT_CASES, "ULA_CASES": tgrad.ULA_CASES, "GRAD_CASES": tuha.GRAD_CASES}
    seen = set()
    for cid, family, builder in cc.CASES:
        got = builder.resolve()
        seen.add(builder.source)
        if builder.source in lists:
            assert got is lists[builder.source][builder.key], cid
            assert (got[0], got[1]) == builder.expect[:2], cid
        elif builder.source == "gc.case_by_id":
            assert got in gc.GATED_CASES and got[0] == builder.key, cid
        elif builder.source == "mc.case_by_id":
            assert got in mc.CASES and got[0] == builder.key, cid
        elif builder.source == "lc.case_by_id":
            assert got in lc.CASES and got[0] == builder.key, cid
        else:
            assert builder.source == "test_lgcp_prepared_tables" and tuple(got) == (230, 2), cid
    assert seen == set(lists) | {"gc.case_by_id", "mc.case_by_id", "lc.case_by_id", "test_lgcp_prepared_tables"}
    # the gated cases of the table are the ones the repeat tests already call twenty times
    repeat = {(c[0], c[4]) for c in tgrad.REPEAT_CASES if c[0].startswith("gated:")}
    assert {("gated:floor-mid", 0), ("gated:clamp-dds-gmm", 1)} <= repeat
    assert cc.case_by_id("gated-floor-mid-item0")[2].item == 0 and cc.case_by_id("gated-clamp-dds-gmm-item1")[2].item == 1


def test_the_item_and_variant_pins_are_the_parity_tests_own():
    """(variant, item) pairs of the table occur in the parametrisation of the parity test of the same list."""
    import test_gpu_grad as tgrad
    def pairs(fn):
        mark = next(m for m in fn.pytestmark if m.name == "parametrize" and m.args[0] == "variant,item")
        return set(mark.args[1])
    allowed = {"BPTT_CASES": pairs(tgrad.test_reparameterised_gradient_matches_autograd),
               "ULA_CASES": pairs(tgrad.test_ula_sn_gradient_matches_autograd)}
    for cid, _, b in cc.CASES:
        if b.source in allowed and b.entry != "MCD_ULA":
            assert (b.variant, b.item) in allowed[b.source], cid
        elif b.source in ("CASES", "GRAD_CASES"):
            assert b.variant is None and b.item in (0, 1), cid
    assert cc.case_by_id("ula-many")[2].item is None and cc.case_by_id("ula-many")[2].variant is None


def test_lgcp_cases_reach_what_they_are_there_for():
    lgcp = [c for c in cc.CASES if c[1].startswith("lgcp")]
    assert {c[0] for c in lgcp} == set(cc.LGCP_FACTS)
    for cid, family, builder in lgcp:
        facts = builder.facts()
        assert facts == cc.LGCP_FACTS[cid], (cid, facts)
        if isinstance(builder, cc.LgcpCase):
            case = builder.resolve()
            assert facts["passes"] == lc.passes_of(case[2]) == lc.PASSES[case[0]]
            assert facts["lanes"] <= min(len(facts["passes"]), cc.LGCP_LANES)
        if family == "lgcp_one_stream":
            assert len(facts["passes"]) == 1 and facts["lanes"] == 1 and not facts["side_streams"] and facts["kept"] in (True, None)
    f = cc.LGCP_FACTS
    # one pass each on the no-split-K products (<= 20 rows) and on split-K with kept activations (21 rows)
    assert lc.gemm_of(f["lgcp-n20"]["passes"][0]) == "merged" and lc.gemm_of(f["lgcp-n21"]["passes"][0]) == "split-k"
    assert f["lgcp-n20"]["kept"] and f["lgcp-n21"]["kept"]
    # the forked cases: a second lane, the two-stream recompute, a second pass of the 2nd-order sweep, the wide path
    assert f["lgcp-n33"]["lanes"] == 2 and f["lgcp-fwd-n33"]["lanes"] == 2 and f["lgcp-n33"]["kept"]
    assert f["lgcp-rc-n21"]["kept"] is False and f["lgcp-rc-n21"]["side_streams"] and f["lgcp-rc-n21"]["lanes"] == 1
    assert f["lgcp-uha-n33"]["passes"] == [32, 1] and not f["lgcp-uha-n33"]["side_streams"]
    # the 2nd-order mode's other sequence: pinned by its form, nothing kept, both passes on the caller's stream
    rc = f["lgcp-uha-rc-n33"]
    assert rc["passes"] == [32, 1] and rc["lanes"] == 1 and rc["kept"] is False and not rc["side_streams"] and not rc["wide"]
    assert cc.case_by_id("lgcp-uha-rc-n33")[2].resolve() == lc.case_by_id("uha-rc-n33") and lc.case_by_id("uha-rc-n33")[4] == 3
    assert lc.UHA_ROUTES["uha-rc-n33"] == ("split-k", "recompute") and lc.UHA_ROUTES["uha-n33"] == ("nsk", "kept")
    assert cc.case_by_id("lgcp-uha-rc-n33")[1] == "lgcp_forked_streams"                  # the function that takes > 1 pass
    assert f["lgcp-wide-n230"]["wide"] and not f["lgcp-fwd-n33"]["wide"]
    assert lc.LGCP_PASS == 32 and cc.LGCP_WIDE_MIN > 129


def test_shapes_stay_small():
    """K is 1 - 3 at d = 1600 and at most 8 elsewhere."""
    for cid, family, builder in cc.CASES:
        got = builder.resolve()
        if isinstance(builder, cc.LgcpCase):
            assert 1 <= got[3] <= 3, cid
        elif isinstance(builder, cc.LgcpWideCase):
            assert got[1] <= 3, cid
        elif isinstance(builder, cc.ListCase):
            from cmcd_amd import synthetic
            assert got[2].get("nbridges", synthetic.CONFIGS[got[0]]["nbridges"]) <= 8, cid
        elif isinstance(builder, cc.GatedCase):
            assert got[2]["nbridges"] <= 8, cid
