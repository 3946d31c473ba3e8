"""Float64 NumPy restatement of the reverse-time chain of UHA, Hamiltonian AIS (include/cmcd_hip.h: cmcd_bound_reverse_hais;
cmcd_amd/reverse_hais.py), shared by tests/test_reverse_hais_oracle.py (which pins it on the CPU against the forward restatement
tests/hais_restatement.py on that restatement's own paths) and tests/test_gpu_reverse_hais.py (which holds the device to it).
Written from the arithmetic in the header and reverse_uha_restatement's key functions; the targets, q and the beta grid are oracle/'s.

TEST INFRASTRUCTURE ONLY.  Besides the chain it holds one deliberately WRONG chain the tests keep the device apart from."""
import numpy as np

from oracle import cmcd_oracle as orc
from oracle import prng
from reverse_uha_restatement import reverse_deviates


def log_mom(s, rho):
    """momdist.log_prob: independent normals of scale s, mean 0."""
    dt = rho.dtype.type
    return np.sum(-(rho ** 2) / (dt(2.0) * s * s) - np.log(s) - dt(0.5 * orc.LOG_2PI), -1)


def _chain(seeds, x, params, dim, nbridges, lfsteps, target, dtype, path, inner_half, trace=None):
    dt = np.dtype(dtype).type
    p = orc.cast_params(params, dtype)
    vd = p["vd"]
    K, L = nbridges, lfsteps
    betas = orc.betas_from_grid(p["mgridref_y"], p["gridref_x"], p["target_x"], dtype)
    eps, eta = dt(p["eps"]), dt(p["eta"])
    s = np.exp(p["md"])
    iv = dt(1.0) / (s * s)
    ce = np.sqrt(dt(1.0) - eta * eta)
    two = dt(2.0)
    unfloored = getattr(target, "unfloored", None)

    def grad_u(zz, beta):      # ONE target evaluation per position, as in the kernel; no clip
        if trace is not None:
            trace.setdefault("lp", []).append(np.array(unfloored(zz) if unfloored else target(zz)[0]))
        _, gp = target(zz)
        return dt(-1.0) * (beta * gp + (dt(1.0) - beta) * orc.q_grad(vd, zz))

    with np.errstate(all="ignore"):
        z = np.asarray(x, dtype).copy()
        if path is None:
            n_k, xi = reverse_deviates(seeds, dim, K)
            r = s * n_k.astype(dtype)
        else:
            r = np.asarray(path[K][2], dtype).copy()
        logp, _ = target(z)
        w = np.asarray(logp, dtype)
        floored = np.isneginf(np.asarray(logp, np.float64))
        gu = grad_u(z, betas[K - 1])                  # at z_K, with the beta of the bridge it opens
        for i in range(K - 1, -1, -1):
            beta = betas[i]
            w = w + log_mom(s, r)
            rho = r + eps * gu / two
            for _ in range(L - 1):
                z = z - eps * rho * iv
                rho = rho + eps * grad_u(z, beta) / (two if inner_half else dt(1.0))
            z = z - eps * rho * iv
            # the evaluation that ends this bridge's leap-frog opens the next one's: grad log p and grad log q are the same, the
            # beta differs
            _, gp = target(z)
            if trace is not None:
                trace.setdefault("lp", []).append(np.array(unfloored(z) if unfloored else target(z)[0]))
            gq = orc.q_grad(vd, z)
            rho = rho + eps * (dt(-1.0) * (beta * gp + (dt(1.0) - beta) * gq)) / two          # now (z_i, rho_i)
            w = w - log_mom(s, rho)
            if path is None:
                r = eta * rho + ce * s * xi[:, K - 1 - i, :].astype(dtype)
            else:
                r = np.asarray(path[i][2], dtype).copy()
            if i > 0:
                gu = dt(-1.0) * (betas[i - 1] * gp + (dt(1.0) - betas[i - 1]) * gq)
        w = w - orc.q_log_prob(vd, z)
        w = np.asarray(w, dtype).copy()
        w[~np.isfinite(np.asarray(x, np.float64)).all(1) | floored | np.isnan(w)] = np.inf
    return w.astype(dtype), z.astype(dtype), r.astype(dtype)


def reverse_chain_hais(seeds, x, params, dim, nbridges, lfsteps, target, dtype=np.float64, path=None, trace=None):
    """Per particle, with s = exp(md), L = lfsteps, gU(z, b) = -(b grad log p + (1 - b) grad log q) (no clip):
      z_K = x; r = s normal(R); w = log p(z_K)
      for i = K-1 .. 0:  w += log N(r; 0, s);  rho = r + eps gU(z, beta_i) / 2
                         (L - 1) times: z -= eps rho / s^2; rho += eps gU(z, beta_i)
                         z -= eps rho / s^2; rho += eps gU(z, beta_i) / 2;  w -= log N(rho; 0, s)
                         r = eta rho + sqrt(1 - eta^2) s xi_r, r = K-1-i
      w -= log q(z_0)
    `path` = [(z_i, rho_i, rin_i)] for i = 0 .. K of a forward chain — rin_i the momentum that enters bridge i's refresh (rin_0 =
    s normal(R), rin_K what leaves the last bridge), rho_i the refreshed one (None at K): evaluate the functional on that path
    instead: the chain starts from rin_K and every reversed refresh lands on rin_i; the (z_i, rho_i) are still those the inverted
    leap-frog produces.  `trace` receives log p before many_gmm's floor at every one of the K L + 1 positions, under "lp".
    A row of x with a non-finite entry, a floored log p(x), or a NaN w, gives w = +inf.
    -> (w[N], z_0[N, dim], rho_0[N, dim] = the last r)."""
    return _chain(seeds, x, params, dim, nbridges, lfsteps, target, dtype, path, False, trace)


def reverse_chain_hais_inner_half_kicks(seeds, x, params, dim, nbridges, lfsteps, target, dtype=np.float64):
    """WRONG: every inner kick of the leap-frog a half-kick (at L = 1 it is the right chain: there is no inner kick)."""
    return _chain(seeds, x, params, dim, nbridges, lfsteps, target, dtype, None, True)


def forward_path(seeds, params, dim, nbridges, lfsteps, target, dtype=np.float64):
    """[(z_i, rho_i, rin_i)] for i = 0 .. K of the forward chain (tests/hais_restatement.py's arithmetic) and z_K."""
    dt = np.dtype(dtype).type
    p = orc.cast_params(params, dtype)
    vd = p["vd"]
    betas = orc.betas_from_grid(p["mgridref_y"], p["gridref_x"], p["target_x"], dtype)
    eps, eta = dt(p["eps"]), dt(p["eta"])
    s = np.exp(p["md"])
    iv = dt(1.0) / (s * s)
    e0, n0, xi = prng.particle_noise_uha(np.asarray(seeds), dim, nbridges)
    z = orc.q_sample(vd, e0.astype(dtype))
    rin = s * n0.astype(dtype)

    def grad_u(zz, beta):
        _, gp = target(zz)
        return dt(-1.0) * (beta * gp + (dt(1.0) - beta) * orc.q_grad(vd, zz))

    path = []
    for i in range(nbridges):
        rho = eta * rin + np.sqrt(dt(1.0) - eta * eta) * s * xi[:, i, :].astype(dtype)
        path.append((z, rho, rin))
        r = rho - eps * grad_u(z, betas[i]) / dt(2.0)
        z = z + eps * r * iv
        for _ in range(lfsteps - 1):
            r = r - eps * grad_u(z, betas[i])
            z = z + eps * r * iv
        rin = r - eps * grad_u(z, betas[i]) / dt(2.0)
    path.append((z, None, rin))
    return path


# --------------------------------------------------------------------------- plumbing for hais_restatement.make_params tuples
def run_restatement(params_flat, unflatten, params_fixed, target, seeds, x, dtype=np.float64, chain=reverse_chain_hais, **kw):
    import hais_restatement as hr
    dim, K, L = params_fixed
    return chain(seeds, x, hr.params_numpy(unflatten, params_flat), dim, K, L, target, dtype=dtype, **kw)
