"""Shared test plumbing: run the oracle on the same synthetic inputs as the HIP path."""
import numpy as np

from cmcd_amd import synthetic
from oracle import cmcd_oracle as orc
from oracle import targets as otg


def oracle_target(cfg, lgcp_counts=None):
    m = cfg["model"]
    if m == "gmm":
        return otg.Gmm()
    if m == "funnel":
        return otg.Funnel(10)
    if m == "many_gmm":
        return otg.ManyGmm(n_mixes=int(cfg.get("n_mixes", 40)), loc_scaling=float(cfg.get("loc_scaling", 40.0)))
    if m == "lgcp":
        return otg.Lgcp(lgcp_counts)
    raise KeyError(m)


def run_oracle(built, seeds, dtype=np.float64, reuse=True, lgcp_counts=None):
    cfg = built["cfg"]
    dim, K, mode, spec = built["params_fixed"]
    p = synthetic.oracle_params(built["unflatten"], built["params_flat"])
    return orc.compute_log_elbo_batch(
        np.asarray(seeds), p, dim, K, mode, spec.arch, oracle_target(cfg, lgcp_counts),
        eps_schedule=cfg["eps_schedule"], grad_clipping=cfg["grad_clipping"], dtype=dtype, reuse=reuse)


def compare_losses(l_hip, l_ref, z_hip, z_ref, tag="", *, K, rel_max=None, z_max=None, bars=None):
    """Parity bar of SURVEY.md section 8c / BASELINE.md section 2 (float32 path vs float64 oracle) on all three outputs of
    compute_bound, `(mean, (losses, z))` (/root/reference/src/mcdboundingmachine.py:183-205):
      * identical set of +inf particles; no NaN;
      * batch mean and ln Z within 1e-3 (absolute, relative above 1);
      * per-particle loss: p99 of the relative error <= 5e-3, and the WORST particle <= 1e-3 for chains of K <= 32 bridges,
        <= 0.2 for longer ones (float32 round-off is amplified along a chaotic chain: 0.13 seen at K = 256);
      * z_K (finite particles): p99 of |z - z_ref| <= 1e-3 max(1, p99 |z_ref|), and for K <= 32 every element within 1e-3
        (scaled the same way).
    `K` = bridges of the chain (0 for the mean-field bound).  `rel_max` / `z_max` override the worst-particle bounds for a
    case that needs a looser one: every such case is listed in DESIGN.md section 2 with its measured value.  `bars`: the same
    for the four other bounds, a dict with keys from "mean", "lnz" (each relative to max(1, |reference|)), "rel_p99" and "z_p99"
    (relative to z_scale) replacing 1e-3, 1e-3, 5e-3 and 1e-3; under the same rule (tests/trained_cases.py)."""
    bars = dict(bars or {})
    assert set(bars) <= {"mean", "lnz", "rel_p99", "z_p99"}, bars
    l_hip = np.asarray(l_hip, np.float64)
    l_ref = np.asarray(l_ref, np.float64)
    z_hip = np.asarray(z_hip, np.float64).reshape(len(l_ref), -1)
    z_ref = np.asarray(z_ref, np.float64).reshape(len(l_ref), -1)
    assert not np.isnan(l_hip).any(), f"{tag}: NaN loss"
    inf_h, inf_r = np.isinf(l_hip), np.isinf(l_ref)
    assert np.array_equal(inf_h, inf_r), f"{tag}: +inf particle sets differ: {np.flatnonzero(inf_h != inf_r)}"
    f = ~inf_r
    rel = np.abs(l_hip[f] - l_ref[f]) / np.maximum(1.0, np.abs(l_ref[f]))
    mean_err = abs(l_hip[f].mean() - l_ref[f].mean())
    lnz_err = abs(orc.ln_z(l_hip) - orc.ln_z(l_ref))
    assert not np.isnan(z_hip[f]).any(), f"{tag}: NaN in z of a finite particle"
    zerr = np.abs(z_hip - z_ref)[f]
    z_scale = max(1.0, float(np.quantile(np.abs(z_ref[f]), 0.99)))
    short = K <= 32
    rel_bound = rel_max if rel_max is not None else (1e-3 if short else 0.2)
    report = dict(n=len(l_ref), n_inf=int(inf_r.sum()), K=K, mean_err=mean_err, lnz_err=lnz_err,
                  rel_p50=float(np.median(rel)), rel_p99=float(np.quantile(rel, 0.99)), rel_max=float(rel.max()),
                  z_p99=float(np.quantile(zerr, 0.99)), z_max=float(zerr.max()), z_scale=z_scale, rel_bound=rel_bound)
    assert mean_err <= bars.get("mean", 1e-3) * max(1.0, abs(l_ref[f].mean())), f"{tag}: {report}"
    assert lnz_err <= bars.get("lnz", 1e-3) * max(1.0, abs(orc.ln_z(l_ref))), f"{tag}: {report}"
    assert report["rel_p99"] <= bars.get("rel_p99", 5e-3), f"{tag}: {report}"
    assert report["rel_max"] <= rel_bound, f"{tag}: worst particle: {report}"
    assert report["z_p99"] <= bars.get("z_p99", 1e-3) * z_scale, f"{tag}: z: {report}"
    if short or z_max is not None:
        assert report["z_max"] <= (z_max if z_max is not None else 1e-3 * z_scale), f"{tag}: worst z element: {report}"
    return report


def run_c_oracle(built, seeds):
    """The plain-C restatement (oracle/cmcd_oracle.c) on the same inputs; float32, reference-faithful."""
    from cmcd_amd import _lib as hip_abi
    from cmcd_amd import mcdboundingmachine as mcdbm
    from oracle import c_oracle
    cfg = built["cfg"]
    dim, K, mode, spec = built["params_fixed"]
    un = built["unflatten"]
    desc = hip_abi.Desc(dim=dim, nbridges=K, mode=hip_abi.MODE[mode], arch=hip_abi.ARCH[spec.arch],
                        emb_dim=spec.emb_dim, target=built["target"].target_id,
                        eps_schedule=hip_abi.EPS_SCHEDULE.get(cfg["eps_schedule"], 0),
                        grad_clipping=int(bool(cfg["grad_clipping"])), ngrid=un.shape("mgridref_y")[0] - 1,
                        reserved=0)
    lay = mcdbm._layout(un, spec)
    consts = built["target"].consts_on("cpu")
    return c_oracle.bound(desc, lay, np.asarray(seeds), built["params_flat"].detach().cpu().numpy(),
                          None if consts is None else consts.numpy())


def lgcp_counts_fixture():
    """The 40x40 bin counts of the Finnish pines point set (tests/golden/lgcp_bin_counts.npy: data)."""
    import os
    return np.load(os.path.join(os.path.dirname(__file__), "golden", "lgcp_bin_counts.npy"))


def check_stats(stats, losses, tag=""):
    """The five on-device statistics `{n_finite, sum l, sum l^2, max(-l), sum exp(-l - max)}` against oracle.cmcd_oracle.stats5
    semantics on the losses the device returned, cast to float64 (what the kernels reduce: the check isolates the reduction
    from the chain's round-off), with the three sums taken by math.fsum so that the reference carries no order error.
      * n_finite and the maximum: exactly equal;
      * sum l, sum l^2: exactly equal when not finite (a +inf loss gives +inf, never NaN); finite: within
        (n + 1024) 2^-53 sum |term|, the worst case of ANY float64 summation order (Higham, Accuracy and Stability, 4.2:
        (n - 1) u sum |x_i| to first order; the 1024 absorbs the higher-order terms);
      * sum exp: within (5 n + 1024) 2^-53 max(1, want) — each exp(x), x <= 0, carries at most (|x| e^x + 3 e^x) 2^-53
        < 4 2^-53 absolute, the per-record rescale the same again (together < 5 n 2^-53 after the common factor), the
        summation order n 2^-53 sum; exactly 0.0 for a batch of +inf losses only;
      * what callers derive: ln Z through mcdboundingmachine.ln_z_from_stats and parallel.finalize within 1e-9 absolute of
        oracle.ln_z (exactly -inf for an all-+inf batch), finalize's mean / variance / n_finite from the same bounds.
    The bounds are derived, not measured: a case beyond them is a finding about a record writer or a merge.
    -> dict of the observed errors relative to their scale (rel_sum, rel_sumsq, rel_exp, lnz_err)."""
    import math

    import torch

    from cmcd_amd import mcdboundingmachine as mcdbm
    from cmcd_amd import parallel
    u = 2.0 ** -53
    st = torch.as_tensor(stats).detach().to("cpu", torch.float64).reshape(5)
    got = st.numpy()
    l = np.asarray(torch.as_tensor(losses).detach().cpu().numpy() if hasattr(losses, "detach") else losses, np.float64).ravel()
    n = l.size
    assert n >= 1 and not np.isnan(l).any() and not (l == -np.inf).any(), f"{tag}: stats5 reference needs losses in (-inf, +inf]"
    fin = np.isfinite(l)
    want0, want3 = float(fin.sum()), float(np.max(-l))
    assert got[0] == want0, f"{tag}: n_finite {got[0]} != {want0}"
    assert got[3] == want3, f"{tag}: max(-loss) {got[3]!r} != {want3!r}"
    rep = dict(n=n, n_inf=int(n - want0), rel_sum=0.0, rel_sumsq=0.0, rel_exp=0.0, lnz_err=0.0)
    terms = {1: l[fin], 2: l[fin] * l[fin]}
    for k, name in ((1, "rel_sum"), (2, "rel_sumsq")):
        if not fin.all():
            assert got[k] == np.inf, f"{tag}: stats[{k}] = {got[k]!r} with a +inf loss in the batch, want +inf"
            continue
        want, mag = math.fsum(terms[k]), math.fsum(np.abs(terms[k]))
        bound = (n + 1024) * u * mag
        assert abs(got[k] - want) <= bound, f"{tag}: stats[{k}] = {got[k]!r}, want {want!r}: off by {abs(got[k] - want):.3e} > {bound:.3e}"
        rep[name] = abs(got[k] - want) / mag if mag > 0 else 0.0
    if want0 == 0:
        want4 = 0.0
        assert got[4] == 0.0, f"{tag}: stats[4] = {got[4]!r} for a batch of +inf losses, want 0.0"
    else:
        want4 = math.fsum(np.exp(-l[fin] - want3))
        bound = (5 * n + 1024) * u * max(1.0, want4)
        assert abs(got[4] - want4) <= bound, f"{tag}: stats[4] = {got[4]!r}, want {want4!r}: off by {abs(got[4] - want4):.3e} > {bound:.3e}"
        rep["rel_exp"] = abs(got[4] - want4) / max(1.0, want4)
    # what the callers derive from the five numbers
    lnz_ref = orc.ln_z(l)
    fz = parallel.finalize(st, n)
    for name, lnz in (("ln_z_from_stats", float(mcdbm.ln_z_from_stats(st, n))), ("parallel.finalize", float(fz["ln_z"]))):
        if want0 == 0:
            assert lnz == -np.inf, f"{tag}: {name} = {lnz!r} for a batch of +inf losses, want -inf"
        else:
            assert abs(lnz - lnz_ref) <= 1e-9, f"{tag}: {name} = {lnz!r}, want {lnz_ref!r}"
            rep["lnz_err"] = max(rep["lnz_err"], abs(lnz - lnz_ref))
    assert float(fz["n_finite"]) == want0, f"{tag}: finalize n_finite"
    mean, var = float(fz["mean"]), float(fz["var"])
    if not fin.all():
        assert mean == np.inf and math.isnan(var), f"{tag}: finalize mean / var = {mean!r} / {var!r} with a +inf loss, want inf / nan"
    else:
        s1, a1, s2 = math.fsum(l), math.fsum(np.abs(l)), math.fsum(l * l)
        m_ref = s1 / n
        assert abs(mean - m_ref) <= ((n + 1024) * u * a1 + 2 * u * abs(s1)) / n, f"{tag}: finalize mean {mean!r}, want {m_ref!r}"
        # var = s2 / n - mean^2 in float64: the two sums' bounds, plus the rounding of the quotient, the square and the difference
        v_ref = math.fsum((l - m_ref) ** 2) / n
        tol = (n + 1024) * u * (s2 + 2 * abs(m_ref) * a1) / n + 8 * u * (s2 / n + m_ref * m_ref)
        if abs(v_ref) + tol < 1e7:
            assert abs(var - v_ref) <= tol, f"{tag}: finalize var {var!r}, want {v_ref!r} (tolerance {tol:.3e})"
        elif v_ref - tol > 1e7:
            assert var == 1e7, f"{tag}: finalize var {var!r}, want the clip 1e7"
    return rep
