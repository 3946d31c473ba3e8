"""tests/grad_blocks.py from the float64 restatement alone (no GPU): the cut tiles every leaf once, the float32 gap behind every bar
is the stored one, the blind spot of the per-leaf comparison is a fact of the reference, and three planted slips pass what the GPU
files asserted before and fail `compare_blocks`, which names the block."""
import numpy as np
import pytest
import torch

import grad_blocks as gb
import lgcp_grad_cases as lg
from test_gpu_grad import _compare

ALL = gb.ids()
W132 = "var-many-w132-n80"


def test_case_table():
    assert len(set(ALL)) == len(ALL) and set(ALL) == set(gb.stored_gaps())
    for cid in ALL:
        assert set(gb.stored_gaps()[cid]) == set(gb.param_sets_of(cid)), cid
    assert len(gb.NEW_CASES) <= 8 and set(gb.NEW_CASES) <= set(ALL)
    for cid in gb.NEW_CASES:
        b = gb.build(cid, "sparse")
        assert len(gb.seeds_of(cid)) <= 80 and b["params_fixed"][1] <= 8, cid
    width = lambda cid: gb.build(cid, "sparse")["params_fixed"][3].width
    assert width("var-many-w132-n49") == width("sn-many-w132-n49") == 132 and width("uha-many-w134-n17") == 134
    assert gb.build("sn-funnel-dds-k1", "sparse")["params_fixed"][:2] == (10, 1)
    assert gb.build("sn-gmm-k1", "sparse")["unflatten"].shape("sn", "emb")[0] == 1
    import ldvi_cases
    assert set(gb.ids("ldvi")) == {"ldvi-" + c for c in ldvi_cases.CASES} - {"ldvi-" + c for c in gb.LDVI_LEAF_ONLY}
    assert set(gb.GATED_IDS) == set(gb.ids("gated")) and len(gb.ids("edge")) == 8
    # every row is found again by its values (the GPU files parametrise over the rows)
    for fam in gb.FAMILIES:
        assert [gb.cid_of(fam, *row) for row in gb.rows(fam)] == gb.ids(fam), fam


def _check_extents(un, by, D):
    """Every block of a matrix leaf (values = flat indices) lies inside one 16-column tile, and inside one 16-row tile (W2, W3,
    linear_3, linear_zero: the row tiles of different waves) or one row group of its first layer: the state rows [:D] — z [:D]
    and rho [D:2D] apart where the net reads [z; rho] — against the embedding rows, the last E of W1 or the last 64 of linear_2/w."""
    for path, (off, shape) in un.layout.items():
        if len(shape) != 2 or path[0] != 0 or path[1] != "sn" or path[-1] == "emb" or path[-1] == "timestep_phase":
            continue
        rows, cols = shape
        key = tuple(path[2:])
        first = key == ("nn", 0, 0) or key == ("drift_net/~/linear_2", "w")
        whole_rows = key in (("drift_net/~/linear", "w"), ("drift_net/~/linear_1", "w"))
        if first:
            emb_rows = un.shape("sn", "emb")[1] if key[0] == "nn" else 64
            bounds = sorted({0, D, rows - emb_rows, rows})
            assert rows - emb_rows in (D, 2 * D), (path, shape)
        seen = 0
        for name, a in by.items():
            idx = a.reshape(-1) - off
            if not (0 <= idx[0] < rows * cols):
                continue
            seen += 1
            r, c = idx // cols, idx % cols
            assert c.min() // 16 == c.max() // 16 or key[-2:] in ((2, 0), ("drift_net/~/linear_zero", "w")), (name, "columns")
            if first:
                assert any(lo <= r.min() and r.max() < hi for lo, hi in zip(bounds, bounds[1:])), (name, "row group", bounds)
                lo = max(x for x in bounds if x <= r.min())
                assert (r.min(), r.max() + 1) == (lo, bounds[bounds.index(lo) + 1]), (name, "a whole row group")
            elif not whole_rows:
                assert r.min() // 16 == r.max() // 16, (name, "rows")
        assert seen >= 1, path


@pytest.mark.parametrize("cid", ALL)
def test_block_cuts_tile_each_leaf_exactly_once(cid):
    for ps in gb.param_sets_of(cid):
        b = gb.build(cid, ps)
        un, numel = b["unflatten"], b["params_flat"].numel()
        bl = gb.blocks(un, np.arange(numel, dtype=np.float64))
        names = [name for name, _, _ in bl]
        assert len(set(names)) == len(names)
        hit = np.zeros(numel, np.int64)
        for _, a, covers in bl:
            assert a.size > 0 and covers
            np.add.at(hit, a.reshape(-1).astype(np.int64), 1)
        assert hit.min() == 1 == hit.max()
        # no block crosses a leaf, a 16-unit tile or the state / embedding rows
        by = dict((n, a) for n, a, _ in bl)
        for path, (off, shape) in un.layout.items():
            inside = [a for a in by.values() if off <= a.reshape(-1)[0] < off + max(1, int(np.prod(shape)))]
            assert all(a.max() < off + max(1, int(np.prod(shape))) for a in inside), path
        _check_extents(un, by, b["params_fixed"][0])
    if cid == W132:
        assert by["W1.state[:,128:132]"].shape == (2, 4) and by["W1.emb[:,128:132]"].shape == (130, 4)
        assert by["W2[128:132,128:132]"].shape == (4, 4) and by["W3[128:132]"].shape == (4, 2) and by["b2[128:132]"].shape == (4,)
        assert by["emb[4]"].shape == (130,) and by["mgridref_y[5]"].shape == (1,) and by["vd.mean[1]"].shape == (1,)
        assert len(names) == 18 + 9 + 81 + 9 + 9 + 1 + 5 + 1 + 3 + 6 + 4 + 2
    if cid == "uha-many-w134-n17":
        assert by["W1.z[:,128:134]"].shape == by["W1.rho[:,128:134]"].shape == (2, 6) and "W1.state[:,0:16]" not in by
        assert by["W1.z[:,0:16]"][0, 0] + 2 * 134 == by["W1.rho[:,0:16]"][0, 0]
    if cid in ("uha-gmm-dds-n64", "gated-uha-floor"):      # 2nd-order dds: linear_2/w has 2 D + 64 rows, three writers' row groups
        assert b["unflatten"].shape("sn", "drift_net/~/linear_2", "w") == (68, 64) and "linear_2.w.state[:,0:16]" not in by
        assert by["linear_2.w.z[:,0:16]"].shape == by["linear_2.w.rho[:,0:16]"].shape == (2, 16)
        assert by["linear_2.w.time[:,0:16]"].shape == by["linear_2.w.time[:,48:64]"].shape == (64, 16)
        assert by["linear_2.w.z[:,0:16]"][0, 0] + 2 * 64 == by["linear_2.w.rho[:,0:16]"][0, 0]
        assert by["linear_2.w.rho[:,0:16]"][0, 0] + 2 * 64 == by["linear_2.w.time[:,0:16]"][0, 0]
    if cid == "sn-funnel-dds-k1":
        assert by["linear_2.w.state[:,0:16]"].shape == (10, 16) and by["linear_2.w.time[:,48:64]"].shape == (64, 16)
        assert by["linear_3.w[16:32,32:48]"].shape == (16, 16) and by["linear_zero.w[48:64]"].shape == (16, 10)
        assert by["linear.w[:,0:16]"].shape == (128, 16) and by["timestep_phase"].shape == (64,) and by["linear_zero.b"].shape == (10,)


@pytest.mark.parametrize("cid,param_set", gb.records())
def test_float32_gap_is_the_stored_one(cid, param_set):
    """tests/test_oracle_lgcp_grad.py's rules on this table: a listed block within 1.5 x of its stored gap, an unlisted one below
    1.5 x LISTED, every bar at least FACTOR x the gap, the losses and z within a quarter of compare_losses' 1e-3, the named tiny /
    zero blocks the same, and no more than MAX_LOST of the blocks lost.
    Two things follow the code path the BLAS takes on the CPU at hand, as measured under two of them (the golden file keeps the
    larger value per entry: `grad_blocks.py --write`, then `--merge`).  The loss and z gaps are a few float32 roundings (1e-7 ..
    4e-5) and moved by up to 2.4 x: a stored one below tests/hais_lgcp_cases.py's GAP_FLOOR counts as GAP_FLOOR, as there.  And
    where the gap sets the bar the stored value may not overstate the re-measured one by more than 1.5 x 1.5: one 1.5 x for the
    re-measurement, one for the other measurement, which the file may hold instead (64 blocks are above a quarter of BAR; the two
    measurements differ by at most 1.73 x there, by more than 1.5 x on two of them, both below 7e-4)."""
    from hais_lgcp_cases import GAP_FLOOR
    gap, stored = gb.float32_gap(cid, param_set), gb.stored_gap(cid, param_set)
    worst = sorted(gap["blocks"].items(), key=lambda kv: -kv[1])[:3]
    print(cid, param_set, "loss %.2e z %.2e" % (gap["loss"], gap["z"]), "worst blocks", [(k, "%.1e" % v) for k, v in worst])
    assert gap["tiny"] == stored["tiny"] and gap["zero"] == stored["zero"]
    assert gap["loss"] <= 1.5 * max(stored["loss"], GAP_FLOOR) and gap["z"] <= 1.5 * max(stored["z"], GAP_FLOOR)
    assert stored["loss"] <= gb.QUARTER * 1e-3 and stored["z"] <= gb.QUARTER * 1e-3
    bar, lost = gb.bars(cid, param_set)
    assert set(stored["blocks"]) <= set(gap["blocks"])
    for name, g in gap["blocks"].items():
        s = stored["blocks"].get(name)
        if s is None:
            assert g <= 1.5 * gb.LISTED, (name, g)
            assert bar(name) == gb.BAR
            continue
        assert s > gb.LISTED and g <= 1.5 * s, (name, g, s)
        if s > gb.QUARTER * gb.BAR:                 # the gap sets the bar (or loses the block): not overstated either
            assert s <= 1.5 * 1.5 * g, (name, g, s)
        if name not in lost:
            assert s <= gb.QUARTER * bar(name) and (bar(name) == gb.BAR or bar(name) == gb.FACTOR * s), (name, s, bar(name))
    nblocks = len(gap["blocks"]) + len(gap["zero"])
    assert len(lost) <= gb.MAX_LOST * nblocks, (lost, nblocks)


def test_the_rule_is_the_d1600_one():
    assert (gb.BAR, gb.QUARTER, gb.FACTOR, gb.LISTED, gb.LOST, gb.MAX_LOST, gb.TINY) == (2e-3, 0.25, 4.0, 1e-4, 5e-2, 0.1, 1e-12)
    assert gb.bar_of is lg.bar_of and gb.bar_of(4e-4) == 2e-3 and gb.bar_of(1e-3) == 4e-3 and gb.bar_of(6e-2) is None


# ------------------------------------------------------------------------------------------ the blind spot and the slips
def _leaf(un, flat, *key):
    off, shape = un.layout[(0,) + key]
    return flat[off:off + max(1, int(np.prod(shape)))].reshape(shape)


def _passes_today(cid, param_set, un, g, g_ref):
    """tests/test_gpu_grad.py:_compare as it stood (no blocks): the 2e-3 leaf bar and the cosine."""
    try:
        _compare(cid, param_set, un, torch.tensor(g), torch.tensor(g_ref))
    except AssertionError:
        return False
    return True


def _block_failures(cid, param_set, un, g, g_ref):
    return gb.compare_blocks(cid, param_set, un, g, g_ref)[1]


@pytest.mark.parametrize("param_set", gb.PARAM_SETS)
def test_embedding_rows_of_dw1_hide_below_the_leaf_bar(param_set):
    """The 132-wide VarGrad case: the 130 embedding rows of dW1 (98 % of the leaf) lie below 2e-3 of the leaf's maximum, which
    the two state rows hold; dropping them costs the cosine less than 1e-7."""
    un = gb.build(W132, param_set)["unflatten"]
    g = gb.reference(W132, param_set)[3]
    W1 = np.abs(_leaf(un, g, "sn", "nn", 0, 0))
    share = W1[2:].max() / W1.max()
    print(W132, param_set, "embedding rows / leaf maximum %.2e" % share)
    assert W1.shape == (132, 132) and W1[:2].max() == W1.max() and 0 < share < 2e-3
    cut = g.copy()
    _leaf(un, cut, "sn", "nn", 0, 0)[2:] = 0.0
    assert 1 - float(cut @ g) / float(np.linalg.norm(cut) * np.linalg.norm(g)) < 1e-7
    rel = {n: np.abs(a).max() / W1.max() for n, a, _ in gb.blocks(un, g) if n.startswith("W1.emb")}
    assert len(rel) == 9 and max(rel.values()) == share


ZEROED_ROWS = ["var-many-w132-n80", "var-many-w132-n49", "var-many-e20-n64", "var-many-e40-n60", "var-many-e70-n40", "sn-many-e20-n64"]


@pytest.mark.parametrize("param_set", gb.PARAM_SETS)
@pytest.mark.parametrize("cid", ZEROED_ROWS)
def test_slip_zeroed_embedding_rows_of_dw1(cid, param_set):
    """A geffner tail that wrote zeros into dW1[D:]: passes the leaf bar and the cosine, fails every W1.emb block."""
    b = gb.build(cid, param_set)
    un, D = b["unflatten"], b["params_fixed"][0]
    g_ref = gb.reference(cid, param_set)[3]
    g = g_ref.copy()
    _leaf(un, g, "sn", "nn", 0, 0)[D:] = 0.0
    assert _passes_today(cid, param_set, un, g, g_ref)
    bad = _block_failures(cid, param_set, un, g, g_ref)
    tiles = [n for n, _, _ in gb.blocks(un, g) if n.startswith("W1.emb")]
    assert len(bad) == len(tiles) and all(any(t + ":" in m for m in bad) for t in tiles), bad


def _last_evaluation_of_emb(cid, param_set):
    """The share of evaluation e = K in d emb[K - 1], from a second run of the reference whose table has a row K (a copy of row
    K - 1; the net clamps its time index to the last row): that row's gradient."""
    def extend(p):
        p["sn"]["emb"] = np.concatenate([p["sn"]["emb"], p["sn"]["emb"][-1:]], 0)
    g2 = gb.run_restatement(cid, param_set, params_edit=extend)[4]["sn"]["emb"]
    return g2[-2], g2[-1]


@pytest.mark.parametrize("param_set", gb.PARAM_SETS)
@pytest.mark.parametrize("cid", [c for c in gb.ids("edge") if c != "edge-var-n1-k1"])
def test_slip_last_evaluation_left_out_of_emb(cid, param_set):
    """d emb[K - 1] without the evaluation e = K.  The per-leaf bar sees it (the share is 5e-2 of the leaf and more), but
    test_gradient_edge_shapes, which holds the flat gradient to 3e-3 of its largest entry, does not: emb is 1e-3 of that entry and
    less.  compare_blocks names the row."""
    b = gb.build(cid, param_set)
    un, K = b["unflatten"], b["params_fixed"][1]
    g_ref = gb.reference(cid, param_set)[3]
    kept, left_out = _last_evaluation_of_emb(cid, param_set)
    g = g_ref.copy()
    row = _leaf(un, g, "sn", "emb")[K - 1]
    assert np.abs(kept + left_out - row).max() <= 1e-9 * np.abs(row).max()       # the second run splits the row, nothing else
    row -= left_out
    assert np.abs(left_out).max() > 5e-2 * np.abs(_leaf(un, g_ref, "sn", "emb")).max()
    assert np.abs(g - g_ref).max() <= 3e-3 * np.abs(g_ref).max()                  # the assertion of test_gradient_edge_shapes
    assert not _passes_today(cid, param_set, un, g, g_ref)
    bad = _block_failures(cid, param_set, un, g, g_ref)
    assert len(bad) == 1 and "emb[%d]:" % (K - 1) in bad[0], bad


SCALED_TILE = [("var-many-w132-n80", "sparse"), ("var-many-w132-n49", "sparse"), ("sn-many-w132-n49", "sparse"),
               ("gated-clip-pq-1e2", "sparse"), ("gated-clip-pq-1e2", "dense")]


@pytest.mark.parametrize("cid,param_set", SCALED_TILE)
def test_slip_one_tile_of_dw2_scaled(cid, param_set):
    """The smallest 16 x 16 tile of dW2 times 0.9 (a wave that lost a tenth of its row tile): below 2e-2 of the leaf's maximum
    on the 132-wide net, so the leaf bar passes a 10 % error; the tile's own bar does not."""
    un = gb.build(cid, param_set)["unflatten"]
    g_ref = gb.reference(cid, param_set)[3]
    g = g_ref.copy()
    W2 = _leaf(un, g, "sn", "nn", 1, 0)
    tiles = [(np.abs(W2[r0:r1, c0:c1]).max(), r0, r1, c0, c1) for r0, r1 in gb._tiles(132) for c0, c1 in gb._tiles(132)]
    m, r0, r1, c0, c1 = min(tiles)
    assert 0 < m < 2e-2 * np.abs(W2).max()
    W2[r0:r1, c0:c1] *= 0.9
    assert _passes_today(cid, param_set, un, g, g_ref)
    bad = _block_failures(cid, param_set, un, g, g_ref)
    assert len(bad) == 1 and "W2[%d:%d,%d:%d]:" % (r0, r1, c0, c1) in bad[0], bad


def test_an_exact_gradient_passes_and_a_zero_block_must_stay_zero():
    un = gb.build(W132, "dense")["unflatten"]
    g_ref = gb.reference(W132, "dense")[3]
    rep, bad = gb.compare_blocks(W132, "dense", un, g_ref.astype(np.float32), g_ref)
    assert not bad and 0 < max(rep.values()) < 1e-6
    g = g_ref.copy()
    g[un.offset("eta")] = 1e-30
    assert any("eta: expected exactly zero" in m for m in gb.compare_blocks(W132, "dense", un, g, g_ref)[1])
