"""Sequential Monte Carlo over the annealing path: the forward chain run in resumable segments, with the particles of a seed
group resampled between bridges when their effective sample size drops.

`segment` is ONE call of libcmcd_hip.so (cmcd_bound_segment, csrc/cmcd_segment.hip): bridges [k0, k1) from q (k0 == 0) or from
the state an earlier segment returned.  A state is a dict of device tensors
    z[N, dim] f32, wpath[N] f32, lg[N] f32, key[N, 2] int32 (the uint32 words of the chain key gen_k), stats[5] f64, k
where wpath is the path weight WITHOUT the end point's density and lg = log gamma_k(z), so that -(wpath + lg) is the loss of a
chain that stopped at bridge k (at k = K: the loss `bound_forward` returns).  Segments compose bit for bit.
`resample_stage` resamples the triggered groups of a state (cmcd_amd.resample, systematic scheme) and `smc_bound` drives the
whole chain.  Nothing here reads a device value back to the host, so a stage can be captured into a graph.  The reference has no
counterpart; the arithmetic is restated in float64 NumPy in tests/smc_restatement.py.  No CPU fallback.  (What the call shares
with the segments of the momentum modes is in cmcd_amd._chain.)"""
import ctypes as C

from . import _chain, _lib
from . import mcdboundingmachine as mcdbm
from ._chain import default_cuts, losses_of      # noqa: F401  (names of this module)

STATE_FIELDS = ("z", "wpath", "lg", "key")


def segment(state, k0, k1, params_flat, unflatten, params_fixed, log_prob, eps_schedule=None, grad_clipping=False):
    """Bridges [k0, k1) of the forward chain, one library call on the current stream.  `state` is `seeds[N]` at k0 == 0 (the chain
    then starts from q exactly as `bound_forward`), otherwise the state of the previous stage, which is left untouched.
    -> the state at bridge k1 (see the module text); its `stats` are the five statistics over -(wpath + lg).
    Overdamped modes on gmm / funnel / many_gmm only (NotImplementedError otherwise)."""
    plan = mcdbm._plan(unflatten, params_fixed, log_prob, eps_schedule, grad_clipping)
    k0, k1 = int(k0), int(k1)
    L, desc = _lib.lib(), C.byref(plan.desc)
    # (the refusal says where MCD_CAIS_UHA_sn's segments are)
    hint = " — MCD_CAIS_UHA_sn: cmcd_amd.smc_uha (the state with momentum)" if params_fixed[2] == "MCD_CAIS_UHA_sn" else None
    return _chain.segment_call(
        state, k0, k1, params_flat, params_fixed[0], False,
        "a segment with k0 > 0 starts from the state dict an earlier segment (or resample_stage) returned",
        "seg", "no segment kernel for this configuration", True, L.cmcd_segment_workspace_bytes, (desc,), plan.desc_b,
        L.cmcd_bound_segment, (desc, C.byref(plan.lay), k0, k1), log_prob.consts_on, params_first=True, hint=hint)


def resample_stage(state, groups=1, ess_threshold=0.5, seed=0):
    """One resampling stage at a cut, per seed group of m = N / groups rows, all on the device (no host read):
    a group is resampled when its ESS < ess_threshold * m, it is not diverged (a NaN or -inf loss) and holds a finite loss.
    A resampled group hands its ln Z column (logsumexp(wpath + lg) - log m) to the running sum, takes z from its ancestors
    (systematic scheme, `resample.resample(..., seed=seed)`) and restarts with uniform weights: wpath_j = -lg[a_j], finite
    because ancestors have positive weight.  KEYS STAY WITH THEIR SLOT: they are not gathered, so two offspring of one ancestor
    draw different noise from here on.  Every other group is passed through unchanged (identity ancestors).
    -> (new state, {"resampled"[groups] bool, "ess"[groups], "ln_Z_increment"[groups] f64, "ancestors"[N] int64})."""
    return _chain.resample_stage(state, groups, ess_threshold, seed)


def smc_bound(seeds, params_flat, unflatten, params_fixed, log_prob, eps_schedule=None, grad_clipping=False, *, groups=1,
              cuts=None, ess_threshold=0.5, seed=0, trace=False):
    """The chain of `bound_forward` with resampling stages at the bridges `cuts` (ascending, inside (0, K); default
    `default_cuts(K)`).  Rows are `groups` consecutive seed groups, each its own particle system; the stage at cut c uses
    `resample_stage(..., seed=seed + c)`.  -> dict of device tensors
        ln_Z[groups] f64     sum of the resampled stages' ln Z columns + logsumexp(wpath + lg) - log m at K
        losses[N] f32        -(wpath + lg) at K: the weights of the final cloud are exp(-losses) within each group
        z[N, dim] f32
        resampled[len(cuts), groups] bool, ess[len(cuts) + 1, groups] f64 (at every cut before resampling, then at K)
    and with trace=True "trace": per stage {"k", "wpath", "lg", "ancestors"} — the state as it ARRIVED at the cut (or at K, where
    ancestors is None).  With ess_threshold = 0 nothing is resampled and losses are the single segment [0, K)'s, bit for bit.
    Each segment runs the prep launch and evaluates its first state again (one extra evaluation per cut).  No host read."""
    return _chain.drive(segment, False, seeds, params_flat, unflatten, params_fixed, log_prob, eps_schedule, grad_clipping, groups,
                        cuts, ess_threshold, seed, trace)
