"""The reverse-time chain (include/cmcd_hip.h: cmcd_bound_reverse; cmcd_amd.mcdboundingmachine.bound_reverse) against a
float64 NumPy restatement built from the pieces oracle/ exports.  The reference has no such call: the yardstick is
`reverse_chain` below, which tests/test_reverse_oracle.py pins without a device (against the forward oracle on its own paths).

Parity goes through helpers.compare_losses / check_stats unchanged (w in the place of the loss, z_0 in the place of z_K)."""
import ctypes as C

import numpy as np
import pytest
import torch

from cmcd_amd import _lib, synthetic
from cmcd_amd import mcdboundingmachine as mcdbm
from cmcd_amd.model_handler import exact_target_draws, load_model
from helpers import check_stats, compare_losses, oracle_target
from oracle import cmcd_oracle as orc
from oracle import prng

# Seeds of the bracket test: the forward call runs on seeds 1 .. 4096 (synthetic.parity_seeds), the reverse call on seeds
# 100001 .. 104096 with the target draws of generator seed 11.  Verified on the CPU with the forward oracle and `reverse_chain`
# (float64) before they were fixed here: forward mean(-loss) = -2.8035 (se 0.0352), reverse mean(w) = +4.5690 (se 0.0685).
BRACKET_N = 4096
BRACKET_REVERSE_SEED0 = 100001
BRACKET_DRAW_SEED = 11


# --------------------------------------------------------------------------- the restatement
def reverse_chain(seeds, x, params, dim, nbridges, mode, arch, target, eps_schedule=None, grad_clipping=False,
                  dtype=np.float64, path=None):
    """Per particle: z_K = x, w = log p(z_K); for i = K-1 .. 0: z_i ~ B_i(. | z_{i+1}) with the r-th deviate of the forward
    call's key chain (r = K-1-i; oracle.prng.particle_noise), w += log B_i(z_i | z_{i+1}) - log F_i(z_{i+1} | z_i);
    w -= log q(z_0).  F_i, B_i, the schedules and the clip rule are those of oracle.cmcd_oracle.compute_log_elbo_batch
    (mcd_cais.py:46-89, mcd_cais_var.py:33-40, mcd_over_orig.py).  `path` = [z_0, .., z_K] (z_K = x): evaluate the functional on
    that path instead — the deviates are then the path's own increments (z_i - m_b) / sigma_i.
    A row of x with a non-finite entry, or a NaN w, gives w = +inf.  -> (w[N], z_0[N, dim]) in `dtype`."""
    dt = np.dtype(dtype).type
    p = orc.cast_params(params, dtype)
    vd, sn = p["vd"], p.get("sn")
    K = nbridges
    betas = orc.betas_from_grid(p["mgridref_y"], p["gridref_x"], p["target_x"], dtype)
    eps_tab = orc.eps_table(p["eps"], K, eps_schedule, dtype)
    var_mode = mode == "MCD_CAIS_var_sn"
    clip = dt(1e2) if var_mode else dt(1e3)
    ula = mode in ("MCD_ULA", "MCD_ULA_sn")
    if ula:
        grad_clipping = False
        eps_tab = np.full(K, dt(p["eps"]), dtype)
    if path is None:
        _, xi = prng.particle_noise(np.asarray(seeds), dim, K)

    def grad_u(zz, beta):
        _, gp = target(zz)
        gq = orc.q_grad(vd, zz)
        if grad_clipping:
            gp = np.clip(gp, -clip, clip)
            if var_mode:
                gq = np.clip(gq, -clip, clip)
        return dt(-1.0) * (beta * gp + (dt(1.0) - beta) * gq)

    with np.errstate(all="ignore"):
        z = np.asarray(x, dtype).copy()
        w, _ = target(z)
        w = np.asarray(w, dtype).copy()
        for i in range(K - 1, -1, -1):
            beta, eps = betas[i], eps_tab[i]
            scale = np.sqrt(dt(2.0) * eps)
            m_b = z - eps * grad_u(z, beta)
            if mode != "MCD_ULA":
                m_b = m_b + eps * orc.apply_sn(arch, sn, z, i if ula else i + 1, dtype)
            dev = xi[:, K - 1 - i, :].astype(dtype) if path is None else (np.asarray(path[i], dtype) - m_b) / scale
            z_new = m_b + scale * dev
            m_f = z_new - eps * grad_u(z_new, beta)
            if not ula:
                m_f = m_f - eps * orc.apply_sn(arch, sn, z_new, i, dtype)
            w = w + (orc.log_prob_kernel(z_new, m_b, scale) - orc.log_prob_kernel(z, m_f, scale))
            z = z_new
        w = w - orc.q_log_prob(vd, z)
        w[~np.isfinite(np.asarray(x, np.float64)).all(1) | np.isnan(w)] = np.inf
    return w.astype(dtype), z.astype(dtype)


def oracle_params(b):
    """synthetic.oracle_params, also for MCD_ULA (whose parameter tree keeps no network)."""
    if b["params_fixed"][2] != "MCD_ULA":
        return synthetic.oracle_params(b["unflatten"], b["params_flat"])
    train, notrain = b["unflatten"](b["params_flat"].detach().cpu())
    allp = {**train, **notrain}
    f = lambda t: np.asarray(t.numpy(), np.float64)
    return {"vd": {k: f(v) for k, v in allp["vd"].items()}, "eps": f(allp["eps"]), "mgridref_y": f(allp["mgridref_y"]),
            "gridref_x": f(allp["gridref_x"]), "target_x": f(allp["target_x"])}


def run_restatement(b, seeds, x, dtype=np.float64):
    dim, K, mode, spec = b["params_fixed"]
    arch = spec.arch if spec is not None else "dds"
    return reverse_chain(seeds, x, oracle_params(b), dim, K, mode, arch, oracle_target(b["cfg"]),
                         eps_schedule=b["cfg"]["eps_schedule"], grad_clipping=b["cfg"]["grad_clipping"], dtype=dtype)


def target_draws(b, n, seed=5):
    cfg = b["cfg"]
    sampler = load_model(cfg["model"], None)[2]
    return exact_target_draws(cfg["model"], sampler, seed, n, b["params_fixed"][0])


def run_device(b, seeds, x):
    xs = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()
    w, z0, st = mcdbm.bound_reverse(torch.from_numpy(np.asarray(seeds, np.int32)).cuda(), xs, b["params_flat"], b["unflatten"],
                                    b["params_fixed"], b["target"], eps_schedule=b["eps_schedule"],
                                    grad_clipping=b["grad_clipping"])
    torch.cuda.synchronize()
    return w, z0, st


def bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64)


# --------------------------------------------------------------------------- parity
# (id, config, overrides, n, dense): every n of {1, 15, 16, 17, 33, 300}, K of {1, 2, 8, 32}, the three targets, geffner
# widths 22 / 58 / 132 and dds 64, the four modes, the three eps schedules, clipping on and off, both parameter sets.
PARITY = [
    ("gmm-w22-cais-k8-n300", "gmm_n300_k8", {}, 300, False),
    ("gmm-w22-cais-k1-n1", "gmm_n300_k8", dict(nbridges=1), 1, True),
    ("gmm-w22-ula_sn-k2-n15", "gmm_n300_k8", dict(boundmode="MCD_ULA_sn", nbridges=2), 15, True),
    ("gmm-ula-k8-n17", "gmm_n300_k8", dict(boundmode="MCD_ULA"), 17, False),
    ("gmm-dds-linear-k2-n16", "gmm_n300_k8", dict(nn_arch="dds", nbridges=2, eps_schedule="linear"), 16, True),
    ("funnel-w58-cos-k32-n33", "funnel_n300_k64", dict(nbridges=32), 33, True),
    ("funnel-dds-linear-clip-k8-n16", "funnel_n300_k64", dict(nn_arch="dds", nbridges=8, eps_schedule="linear",
                                                            grad_clipping=True), 16, False),
    ("many_gmm-w132-var-clip-k8-n33", "many_gmm_var_n16000_k256", dict(nbridges=8), 33, True),
    ("many_gmm-w132-cais-k2-n17", "many_gmm_var_n16000_k256", dict(boundmode="MCD_CAIS_sn", nbridges=2, grad_clipping=False),
     17, False),
    ("many_gmm-dds-cos-clip-k32-n300", "many_gmm_n2000_k256_dds", dict(nbridges=32), 300, False),
    ("many_gmm-dds-ula_sn-k8-n33", "many_gmm_n2000_k256_dds", dict(boundmode="MCD_ULA_sn", nbridges=8, init_eps=0.05), 33, True),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", PARITY, ids=[c[0] for c in PARITY])
def test_parity_with_the_restatement(case):
    tag, name, over, n, dense = case
    b = synthetic.build(name, device="cuda", dense=dense, **over)
    K = b["params_fixed"][1]
    seeds = synthetic.parity_seeds(n) + 40
    x = target_draws(b, n)
    w, z0, st = run_device(b, seeds, x)
    w_ref, z_ref = run_restatement(b, seeds, x)
    print(tag, "w[:4]", w[:4].cpu().numpy(), "ref", w_ref[:4])
    print(tag, compare_losses(w.cpu().numpy(), w_ref, z0.cpu().numpy(), z_ref, tag, K=K))
    print(tag, check_stats(st, w, tag))
    eubo, _ = mcdbm.compute_reverse_bound(torch.from_numpy(seeds).cuda(), torch.from_numpy(x).cuda(), b["params_flat"],
                                          b["unflatten"], b["params_fixed"], b["target"], eps_schedule=b["eps_schedule"],
                                          grad_clipping=b["grad_clipping"])
    assert abs(float(eubo) - w_ref.mean()) <= 1e-3 * max(1.0, abs(w_ref.mean()))


@pytest.mark.gpu
def test_ula_sn_takes_the_network_at_index_i():
    """MCD_ULA_sn's backward mean uses s(z_{i+1}, i), not s(z_{i+1}, i + 1) (mcd_over_orig.py): a restatement with the CAIS
    index must NOT match, on parameters where the per-bridge embedding matters."""
    b = synthetic.build("gmm_n300_k8", device="cuda", dense=True, boundmode="MCD_ULA_sn", nbridges=4, init_eps=0.05)
    p = synthetic.oracle_params(b["unflatten"], b["params_flat"])
    p["sn"]["emb"] = p["sn"]["emb"] * 40.0          # make the bridge index count
    flat = b["params_flat"].clone()
    off, shape = b["unflatten"].layout[(0, "sn", "emb")]
    flat[off:off + int(np.prod(shape))] *= 40.0
    b = dict(b, params_flat=flat)
    n = 33
    seeds, x = synthetic.parity_seeds(n), target_draws(b, n)
    w, z0, _ = run_device(b, seeds, x)
    w_ref, z_ref = run_restatement(b, seeds, x)
    compare_losses(w.cpu().numpy(), w_ref, z0.cpu().numpy(), z_ref, "ula_sn index", K=4)

    shifted = dict(p["sn"], emb=np.roll(p["sn"]["emb"], -1, axis=0))     # row i of this table is row i + 1 of the real one
    w_bad, _ = reverse_chain(seeds, x, dict(p, sn=shifted), 2, 4, "MCD_ULA_sn", "geffner", oracle_target(b["cfg"]))
    assert np.abs(w_bad - w_ref).max() > 1e-2


@pytest.mark.gpu
def test_parity_far_out_in_the_tail():
    """x far from the mass: grad log p exceeds the clip (the gmm's precision 20 x a distance of ~150), w spans thousands."""
    b = synthetic.build("gmm_n300_k8", device="cuda", dense=True, grad_clipping=True)
    n = 17
    seeds = synthetic.parity_seeds(n)
    x = target_draws(b, n) + np.linspace(20.0, 160.0, n, dtype=np.float32)[:, None] * np.array([1.0, -0.9], np.float32)
    _, gp = oracle_target(b["cfg"])(x.astype(np.float64))
    assert (np.abs(gp) > 1e3).any()
    w, z0, st = run_device(b, seeds, x)
    w_ref, z_ref = run_restatement(b, seeds, x)
    print("tail w", w.cpu().numpy())
    assert np.ptp(w_ref) > 2e3
    print(compare_losses(w.cpu().numpy(), w_ref, z0.cpu().numpy(), z_ref, "tail", K=8))
    check_stats(st, w, "tail")


# --------------------------------------------------------------------------- non-finite rows
@pytest.mark.gpu
@pytest.mark.parametrize("whole_tile", [False, True])
def test_non_finite_rows_weigh_nothing(whole_tile):
    b = synthetic.build("many_gmm_n2000_k256_dds", device="cuda", nbridges=8, dense=True)
    n = 49
    seeds = synthetic.parity_seeds(n)
    x = target_draws(b, n)
    clean_w, clean_z, _ = run_device(b, seeds, x)
    bad = [3, 20] + (list(range(32, 48)) if whole_tile else [])
    x = x.copy()
    x[3, 1] = np.nan
    x[20, 0] = np.inf
    for r in bad[2:]:
        x[r, r % 2] = np.nan if r % 3 else -np.inf
    w, z0, st = run_device(b, seeds, x)
    wc, good = w.cpu().numpy(), np.setdiff1d(np.arange(n), bad)
    assert np.all(wc[bad] == np.inf) and not np.isnan(wc).any()
    assert torch.equal(bits(w[good]), bits(clean_w[good])) and torch.equal(bits(z0[good]), bits(clean_z[good]))
    s = st.cpu().numpy()
    assert not np.isnan(s).any() and s[0] == n - len(bad) and s[1] == np.inf
    check_stats(st, w, "non-finite rows")
    eubo, _ = mcdbm.compute_reverse_bound(torch.from_numpy(seeds).cuda(), torch.from_numpy(x).cuda(), b["params_flat"],
                                          b["unflatten"], b["params_fixed"], b["target"], eps_schedule=b["eps_schedule"],
                                          grad_clipping=b["grad_clipping"])
    assert float(eubo) == np.inf


# --------------------------------------------------------------------------- determinism and composition
@pytest.fixture(scope="module")
def funnel_case():
    b = synthetic.build("funnel_n300_k64", device="cuda", nbridges=8, dense=True)
    n = 300
    seeds = torch.from_numpy(synthetic.parity_seeds(n)).cuda()
    x = torch.from_numpy(target_draws(b, n)).cuda()
    args = (b["params_flat"], b["unflatten"], b["params_fixed"], b["target"])
    kw = dict(eps_schedule=b["eps_schedule"], grad_clipping=b["grad_clipping"])
    out = mcdbm.bound_reverse(seeds, x, *args, **kw)
    torch.cuda.synchronize()
    return seeds, x, args, kw, out


@pytest.mark.gpu
def test_repeated_calls_give_equal_bits(funnel_case):
    seeds, x, args, kw, first = funnel_case
    again = mcdbm.bound_reverse(seeds, x, *args, **kw)
    torch.cuda.synchronize()
    for a, c in zip(first, again):
        assert torch.equal(bits(a), bits(c))


@pytest.mark.gpu
def test_a_particle_does_not_depend_on_its_batch(funnel_case):
    seeds, x, args, kw, whole = funnel_case
    rows = torch.arange(100, 117, device="cuda")       # 17 rows that straddle two tiles of the large batch
    w, z0, _ = mcdbm.bound_reverse(seeds[rows].contiguous(), x[rows].contiguous(), *args, **kw)
    torch.cuda.synchronize()
    assert torch.equal(bits(w), bits(whole[0][rows])) and torch.equal(bits(z0), bits(whole[1][rows]))


@pytest.mark.gpu
def test_graph_capture_and_replay(funnel_case):
    seeds, x, args, kw, eager = funnel_case
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        mcdbm.bound_reverse(seeds, x, *args, **kw)      # allocator warm-up on a side stream
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = mcdbm.bound_reverse(seeds, x, *args, **kw)
    for t in captured:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for a, c in zip(eager, captured):
        assert torch.equal(bits(a), bits(c))


@pytest.mark.gpu
def test_non_default_stream(funnel_case):
    seeds, x, args, kw, eager = funnel_case
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out = mcdbm.bound_reverse(seeds, x, *args, **kw)
    side.synchronize()
    for a, c in zip(eager, out):
        assert torch.equal(bits(a), bits(c))


# --------------------------------------------------------------------------- the bracket
@pytest.mark.gpu
def test_elbo_and_eubo_bracket_ln_z():
    """gmm is normalised (ln Z = 0): E_Q[-loss] <= 0 <= E_P[w], each within 4 standard errors of its own sample."""
    b = synthetic.build("gmm_n300_k8", device="cuda", dense=True)
    n = BRACKET_N
    args = (b["params_flat"], b["unflatten"], b["params_fixed"], b["target"])
    kw = dict(eps_schedule=b["eps_schedule"], grad_clipping=b["grad_clipping"])
    loss, _, _ = mcdbm.bound_forward(torch.from_numpy(synthetic.parity_seeds(n)).cuda(), *args, **kw)
    x = torch.from_numpy(target_draws(b, n, seed=BRACKET_DRAW_SEED)).cuda()
    seeds = torch.arange(BRACKET_REVERSE_SEED0, BRACKET_REVERSE_SEED0 + n, dtype=torch.int32, device="cuda")
    w, _, st = mcdbm.bound_reverse(seeds, x, *args, **kw)
    torch.cuda.synchronize()
    f, r = -loss.double().cpu().numpy(), w.double().cpu().numpy()
    se_f, se_r = f.std(ddof=1) / np.sqrt(n), r.std(ddof=1) / np.sqrt(n)
    print("forward mean(-loss) %.4f (se %.4f); reverse mean(w) %.4f (se %.4f); reverse ln Z %.4f" % (
        f.mean(), se_f, r.mean(), se_r, -float(mcdbm.ln_z_from_stats(st, n))))
    assert np.isfinite(f).all() and np.isfinite(r).all()
    assert f.mean() <= 0.0 + 4 * se_f
    assert r.mean() >= 0.0 - 4 * se_r


# --------------------------------------------------------------------------- refusals
@pytest.mark.gpu
def test_unsupported_configurations_raise():
    n = 32
    seeds = torch.arange(1, n + 1, dtype=torch.int32, device="cuda")
    for name, over in (("gmm_n300_k8", dict(boundmode="MCD_CAIS_UHA_sn")),     # 2nd-order CMCD: no reverse kernel
                       ("gmm_n300_k8", dict(emb_dim=200))):                    # width 202: no instance
        b = synthetic.build(name, device="cuda", **over)
        x = torch.zeros((n, 2), device="cuda")
        with pytest.raises(NotImplementedError):
            mcdbm.bound_reverse(seeds, x, b["params_flat"], b["unflatten"], b["params_fixed"], b["target"])
    from helpers import lgcp_counts_fixture
    b = synthetic.build("lgcp_n20_k128", device="cuda", lgcp_counts=lgcp_counts_fixture(), nbridges=2)
    with pytest.raises(NotImplementedError, match="lgcp"):
        mcdbm.bound_reverse(seeds, torch.zeros((n, 1600), device="cuda"), b["params_flat"], b["unflatten"], b["params_fixed"],
                            b["target"])


@pytest.mark.gpu
def test_bad_inputs_fail_before_any_launch():
    b = synthetic.build("gmm_n300_k8", device="cuda")
    n = 32
    seeds = torch.arange(1, n + 1, dtype=torch.int32, device="cuda")
    args = (b["params_flat"], b["unflatten"], b["params_fixed"], b["target"])
    good = torch.zeros((n, 2), device="cuda")
    with pytest.raises(RuntimeError, match="ROCm device"):
        mcdbm.bound_reverse(seeds, good.cpu(), *args)
    with pytest.raises(ValueError, match="shape"):
        mcdbm.bound_reverse(seeds, torch.zeros((n, 3), device="cuda"), *args)
    with pytest.raises(ValueError, match="shape"):
        mcdbm.bound_reverse(seeds, torch.zeros((n + 1, 2), device="cuda"), *args)
    with pytest.raises(ValueError, match="float32"):
        mcdbm.bound_reverse(seeds, good.double(), *args)
    with pytest.raises(ValueError, match="contiguous"):
        mcdbm.bound_reverse(seeds, torch.zeros((2, n), device="cuda").t(), *args)
    # the C level: a workspace one byte short, a null x
    L = _lib.lib()
    plan = mcdbm._plan(b["unflatten"], b["params_fixed"], b["target"], b["eps_schedule"], b["grad_clipping"])
    need = L.cmcd_reverse_workspace_bytes(C.byref(plan.desc), n)
    assert need > 0 and need == L.cmcd_workspace_bytes(C.byref(plan.desc), n)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    w, z0, st = mcdbm._outputs(n, 2, good.device)
    w.fill_(7.0)

    def call(x_ptr, ws_bytes):
        return L.cmcd_bound_reverse(C.byref(plan.desc), C.byref(plan.lay), seeds.data_ptr(), x_ptr, n, b["params_flat"].data_ptr(),
                                    b["params_flat"].numel(), None, 0, ws.data_ptr(), ws_bytes, w.data_ptr(), z0.data_ptr(),
                                    st.data_ptr(), None)

    assert call(good.data_ptr(), need - 1) == -3 and "workspace too small" in _lib.last_error()
    assert call(None, need) == -1 and "null pointer" in _lib.last_error()
    torch.cuda.synchronize()
    assert bool((w == 7.0).all())                 # nothing ran
    assert call(good.data_ptr(), need) == 0
    torch.cuda.synchronize()
    assert bool((w != 7.0).all())
