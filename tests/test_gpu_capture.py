"""The gradient calls the project is used for — and the d = 1600 forward — on a side stream and captured into a graph, against
their own eager bits (tests/capture_cases.py: the protocol, and the table of cases, each one a case a parity test already holds
to float64 autograd).  opt.run(use_graph=True) replays these calls behind the optimiser step with no host synchronisation; the
zeroing sites they pass (hipMemsetAsync in grad_launch, ula_grad_launch, uha_grad_launch, cmcd_mfvi.hip, cmcd_lgcp.hip,
cmcd_lgcp_wide.hip, and the Jacobian launch's own zeroing on the work-item paths) become memset nodes or graph-ordered kernel
nodes there.  DESIGN.md section 2, "Captured and side-stream calls", has the table of sites and the case that reaches each.

LDVI, HAIS, the reverse chains and the segments have capture tests in their own files."""
import pytest

import capture_cases as cc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("cid", cc.ids_of("mcd"))
def test_mcd_gradient(hip_lib, monkeypatch, cid):
    """compute_log_var_grad / compute_bound_grad: VarGrad and the reparameterised gradient on both item paths, MCD_ULA_sn
    (grad_launch with ula = 2), MCD_ULA (ula_grad_launch), floored particles and clamped outputs."""
    cc.run_case(cid, monkeypatch)


@pytest.mark.parametrize("cid", cc.ids_of("uha"))
def test_uha_gradient(hip_lib, monkeypatch, cid):
    """MCD_CAIS_UHA_sn: whole chains (the memsets of uha_grad_launch) and work items, and the floored case."""
    cc.run_case(cid, monkeypatch)


@pytest.mark.parametrize("cid", cc.ids_of("mfvi"))
def test_mfvi(hip_lib, monkeypatch, cid):
    """boundingmachine.grad_and_loss and compute_bound: the tile path, a +inf batch, and lgcp's passes."""
    cc.run_case(cid, monkeypatch)


@pytest.mark.parametrize("cid", cc.ids_of("lgcp_one_stream"))
def test_lgcp_one_stream(hip_lib, monkeypatch, cid):
    """d = 1600 where the whole call stays on the caller's stream: the captured graph is one chain of nodes."""
    assert not cc.LGCP_FACTS[cid]["side_streams"] and len(cc.LGCP_FACTS[cid]["passes"]) == 1
    cc.run_case(cid, monkeypatch)


@pytest.mark.parametrize("cid", cc.ids_of("lgcp_forked_streams"))
def test_lgcp_forked_streams(hip_lib, monkeypatch, cid):
    """d = 1600 beyond one pass or with the recompute: the forward's lanes and the sweep's recompute run on side streams forked
    from and joined to the caller's by events, so the captured graph has parallel branches and the side streams' memsets are
    nodes of it; lgcp_grad and lgcp_uha_grad clear their per-pass accumulators at `base > 0`; the wide-batch forward.  Runs with
    the process's own queue count; sets no environment variable.  (uha-n33, uha-rc-n33 and the wide call stay on one stream: they
    are here for their pass count and their size.  uha-rc-n33 is the 2nd-order mode's split-K forward, whose counter clear is a
    zeroing launch, and its recompute sweep.)"""
    facts = cc.LGCP_FACTS[cid]
    assert facts["side_streams"] or facts["wide"] or len(facts["passes"]) > 1
    cc.run_case(cid, monkeypatch)
