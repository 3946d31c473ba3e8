"""Final-metric arithmetic and the evaluation harness around the hot path.

`log_final_losses` mirrors /root/reference/src/utils.py:219-248 (without the W&B logging);
`sample` mirrors /root/reference/src/opt.py:167-197 — the call sequence whose throughput
BASELINE.json's metric counts — but evaluates all `n_input_dist_seeds * n_samples` particles in ONE
launch sequence instead of a Python loop with a device->host sync per element
(`[x.item() for x in loss_list]`, opt.py:193).
"""
import math

import torch


def log_final_losses(eval_losses, log_prefix=""):
    """eval_losses: [n_input_dist_seeds, n_samples] -> (final_elbo, final_ln_Z) like the reference;
    the standard deviations over seed groups are returned as attributes of the result tuple's
    companion dict via `log_final_losses.last`."""
    e = torch.as_tensor(eval_losses, dtype=torch.float64)
    n_samples = e.shape[1]
    final_elbos = -e.mean(dim=1)
    final_ln_zs = torch.logsumexp(-e, dim=1) - math.log(n_samples)
    out = {
        f"elbo_final{log_prefix}": float(final_elbos.mean()),
        f"final_ln_Z{log_prefix}": float(final_ln_zs.mean()),
        f"elbo_final_std{log_prefix}": float(final_elbos.std(unbiased=False)),   # jnp.std: ddof = 0
        f"final_ln_Z_std{log_prefix}": float(final_ln_zs.std(unbiased=False)),
    }
    log_final_losses.last = out
    return out[f"elbo_final{log_prefix}"], out[f"final_ln_Z{log_prefix}"]


log_final_losses.last = {}


def log_importance_diagnostics(eval_losses, log_prefix=""):
    """eval_losses: [n_input_dist_seeds, n_samples] DEVICE tensor -> the effective sample size of the importance weights
    exp(-loss) behind each group's ln Z, as mean and standard deviation (ddof = 0) over the groups, absolute and as a
    fraction of n_samples.  One launch (cmcd_amd.resample.importance_stats); the reference reports no such figure."""
    from . import resample
    n_groups, n_samples = eval_losses.shape
    ess = resample.importance_stats(eval_losses, groups=n_groups)["ess"]
    out = {
        f"ess{log_prefix}": float(ess.mean()),
        f"ess_std{log_prefix}": float(ess.std(unbiased=False)),
        f"ess_frac{log_prefix}": float(ess.mean()) / n_samples,
        f"ess_frac_std{log_prefix}": float(ess.std(unbiased=False)) / n_samples,
    }
    log_importance_diagnostics.last = out
    return out


log_importance_diagnostics.last = {}


def log_reverse_diagnostics(w_groups, log_prefix=""):
    """w_groups: [n_input_dist_seeds, n_samples] DEVICE tensor of reverse log-weights (mcdboundingmachine.bound_reverse on
    draws from the target) -> per group the EUBO mean(w) >= ln Z, the reverse estimate ln Z = -(logsumexp(-w) - log n_samples)
    and the effective sample size of the reverse importance weights exp(-w); each as mean and standard deviation (ddof = 0)
    over the groups, the ESS also as a fraction of n_samples.  The ESS and ln Z come from one launch
    (cmcd_amd.resample.importance_stats, which reads w as a loss); the reference reports no such figures."""
    from . import resample
    n_groups, n_samples = w_groups.shape
    st = resample.importance_stats(w_groups, groups=n_groups)
    eubo = w_groups.to(torch.float64).mean(dim=1)
    ln_z, ess = -st["ln_Z"], st["ess"]
    out = {
        f"eubo{log_prefix}": float(eubo.mean()),
        f"eubo_std{log_prefix}": float(eubo.std(unbiased=False)),
        f"reverse_ln_Z{log_prefix}": float(ln_z.mean()),
        f"reverse_ln_Z_std{log_prefix}": float(ln_z.std(unbiased=False)),
        f"reverse_ess{log_prefix}": float(ess.mean()),
        f"reverse_ess_std{log_prefix}": float(ess.std(unbiased=False)),
        f"reverse_ess_frac{log_prefix}": float(ess.mean()) / n_samples,
        f"reverse_ess_frac_std{log_prefix}": float(ess.std(unbiased=False)) / n_samples,
    }
    log_reverse_diagnostics.last = out
    return out


log_reverse_diagnostics.last = {}


def log_smc_diagnostics(result, log_prefix=""):
    """result: what cmcd_amd.smc.smc_bound returned -> the SMC estimate of ln Z as mean and standard deviation (ddof = 0) over
    the seed groups, the number of resampling events (group x cut), and the effective sample size of the final weighted cloud
    (mean, standard deviation, and as a fraction of the group size).  The reference reports no such figures."""
    ln_z, ess = result["ln_Z"], result["ess"][-1]
    m = result["losses"].numel() // ln_z.numel()
    out = {
        f"smc_ln_Z{log_prefix}": float(ln_z.mean()),
        f"smc_ln_Z_std{log_prefix}": float(ln_z.std(unbiased=False)),
        f"smc_resampling_events{log_prefix}": int(result["resampled"].sum()),
        f"smc_stages{log_prefix}": int(result["resampled"].numel()),
        f"smc_ess{log_prefix}": float(ess.mean()),
        f"smc_ess_std{log_prefix}": float(ess.std(unbiased=False)),
        f"smc_ess_frac{log_prefix}": float(ess.mean()) / m,
    }
    log_smc_diagnostics.last = out
    return out


log_smc_diagnostics.last = {}


def sample(info, n_samples, n_input_dist_seeds, params_flat, unflatten, params_fixed, log_prob_model, loss_fn,
           eval_seeds, log_prefix=""):
    """/root/reference/src/opt.py:167-197 -> (elbos [n_input_dist_seeds][n_samples], zs [n*m, dim]).

    `eval_seeds` replaces the reference's `jax.random.randint(rng_key_gen, (n,), 1, 1e6)` (opt.py:182):
    an int32 tensor of n_samples * n_input_dist_seeds seeds.  `loss_fn` is called exactly like the
    reference's jitted callable, once, on all seeds; the per-group split happens afterwards."""
    eval_seeds = torch.as_tensor(eval_seeds)
    assert eval_seeds.numel() == n_samples * n_input_dist_seeds
    _, (loss_list, z) = loss_fn(eval_seeds, params_flat, unflatten, params_fixed, log_prob_model)
    elbos = loss_list.view(n_input_dist_seeds, n_samples)
    return elbos, z


def params_to_numpy(params_flat, unflatten):
    """`params = {**params_train, **params_notrain}` (/root/reference/src/main.py:283-284) as nested dicts / lists
    of NumPy arrays — the structure the reference pickles as `params.pkl` (:286-296), minus the jax array type."""
    import numpy as np

    def conv(t):
        if isinstance(t, dict):
            return {k: conv(v) for k, v in t.items()}
        if isinstance(t, (list, tuple)):
            return type(t)(conv(v) for v in t)
        return np.asarray(t.detach().cpu().numpy())
    train, notrain = unflatten(params_flat.detach().cpu())
    return conv({**train, **notrain})


def save_params(path, params_flat, unflatten):
    """Writes `params.pkl` like the reference's W&B artifact (main.py:286-296): one pickle of the merged dict."""
    import pickle
    with open(path, "wb") as f:
        pickle.dump(params_to_numpy(params_flat, unflatten), f)


def load_params(path_or_dict, params_flat, unflatten):
    """Inverse of `save_params`: copies every leaf of a merged `params` dict (a pickle path, or the dict itself,
    e.g. a reference run's `jax.tree_util.tree_map(np.asarray, params)`) into a copy of `params_flat` at the
    offsets of `unflatten`.  Leaves are matched by name and must have the reference's shapes."""
    import pickle
    import numpy as np
    params = path_or_dict
    if not isinstance(params, dict):
        with open(path_or_dict, "rb") as f:
            params = pickle.load(f)
    out = params_flat.detach().clone()

    def walk(node, prefix):
        if isinstance(node, dict):
            for k, v in node.items():
                walk(v, prefix + (k,))
        elif isinstance(node, (list, tuple)):
            for i, v in enumerate(node):
                walk(v, prefix + (i,))
        else:
            arr = np.asarray(node, np.float32)
            hit = [(path, off, shape) for path, (off, shape) in unflatten.layout.items() if path[1:] == prefix]
            if not hit:
                raise KeyError(f"leaf {prefix} is not part of this parameter tree")
            _, off, shape = hit[0]
            if tuple(arr.shape) != tuple(shape):
                raise ValueError(f"leaf {prefix}: shape {arr.shape} != {tuple(shape)}")
            out[off:off + max(arr.size, 1)] = torch.from_numpy(arr.reshape(-1)).to(out.device)
    walk(params, ())
    return out


def W2_distance(x, y, reg=0.01, num_iter_max=10000, stop_thr=1e-16):
    """/root/reference/src/utils.py:207-216: entropic OT cost `ot.sinkhorn2(a, b, M / M.max(), reg)` between two equal-size
    point clouds with uniform weights — the Sinkhorn-Knopp iteration of POT's default solver (POT itself is not in this
    image), in float64 torch on the device of `x`: u <- a / (K v), v <- b / (K^T u), K = exp(-M / reg); stops when the
    marginal violation drops below `stop_thr` (checked every 10 iterations) or after `num_iter_max` iterations."""
    x = torch.as_tensor(x, dtype=torch.float64)
    y = torch.as_tensor(y, dtype=torch.float64, device=x.device)
    n = x.shape[0]
    a = torch.full((n,), 1.0 / n, dtype=torch.float64, device=x.device)
    b = a.clone()
    M = torch.cdist(x, y) ** 2                      # ot.dist default: squared Euclidean
    M = M / M.max()
    Kmat = torch.exp(-M / reg)
    u, v = torch.ones_like(a) / n, torch.ones_like(b) / n
    for it in range(num_iter_max):
        KtU = Kmat.t() @ u
        v = b / KtU
        u = a / (Kmat @ v)
        if it % 10 == 0:
            err = torch.linalg.norm(v * (Kmat.t() @ u) - b) ** 2
            if float(err) < stop_thr:
                break
    P = u[:, None] * Kmat * v[None, :]
    return float((P * M).sum())


def _is_device(t):
    return isinstance(t, torch.Tensor) and t.is_cuda


def calculate_W2_distances(samples, target_samples, other_target_samples, n_samples, n_input_dist_seeds, n_sinkhorn,
                           log_prefix="", batched=None, losses=None, also=None, self_w2=None):
    """/root/reference/src/utils.py:251-282, returning the four numbers it logs to W&B.

    `batched=None` takes the device path when all three clouds are device tensors: cloud -> target and target -> other target
    for every seed group are then solved in ONE `sinkhorn.w2_batched` call (float64 HIP, same arithmetic) instead of
    2 x n_input_dist_seeds `W2_distance` calls; `batched=False` and CPU inputs keep the loop.  Device path only:
    `losses` ([n_input_dist_seeds * n_samples], the evaluation's) adds `w2_weighted_dist[_std]`: the same metric with the cloud's
    rows weighted a = softmax(-loss) within each group, in float64 — the importance-weighted cloud without resampling noise
    (a loss of +inf weighs 0); `also` ({name: cloud}) adds `w2_dist_<name>[_std]` for further clouds against the same target,
    in the same call; `self_w2` (the (mean, std) an earlier call on the same targets returned) skips the target -> other
    target problems."""
    import numpy as np
    assert n_sinkhorn <= n_samples
    if batched is None:
        batched = _is_device(samples) and _is_device(target_samples) and _is_device(other_target_samples)
    if batched:
        from . import sinkhorn
        G = n_input_dist_seeds

        def groups(t):          # [G * n_samples, d] -> the first n_sinkhorn rows of every group
            if not _is_device(t):
                raise RuntimeError("the CMCD hot path runs on a ROCm device only: a cloud is not a device tensor")
            t = t.detach()
            return t.reshape(G, n_samples, -1)[:, :n_sinkhorn].to(torch.float64)
        tgt = groups(target_samples)
        uniform = torch.full((G, n_sinkhorn), 1.0 / n_sinkhorn, dtype=torch.float64, device=tgt.device)
        sets = [("w2_dist", groups(samples), tgt, uniform)]
        if self_w2 is None:
            sets.append(("self_w2_dist", tgt, groups(other_target_samples), uniform))
        for name, cloud in (also or {}).items():
            sets.append((f"w2_dist_{name}", groups(cloud), tgt, uniform))
        if losses is not None:
            w = torch.softmax(-groups(losses.reshape(-1, 1))[:, :, 0], dim=1)
            sets.append(("w2_weighted_dist", sets[0][1], tgt, w))
        res = sinkhorn.w2_batched(torch.cat([s[1] for s in sets]), torch.cat([s[2] for s in sets]),
                                  a=torch.cat([s[3] for s in sets]))
        cost = res["cost"].view(len(sets), G).cpu().numpy()
        out = {}
        for row, s in zip(cost, sets):
            out[f"{s[0]}{log_prefix}"] = float(np.mean(row))
            out[f"{s[0]}_std{log_prefix}"] = float(np.std(row))
        if self_w2 is not None:
            out[f"self_w2_dist{log_prefix}"], out[f"self_w2_dist_std{log_prefix}"] = float(self_w2[0]), float(self_w2[1])
        return out
    if losses is not None or also or self_w2 is not None:
        raise RuntimeError("the CMCD hot path runs on a ROCm device only: losses= / also= / self_w2= belong to the batched path")
    w2, self_w2 = [], []
    for i in range(n_input_dist_seeds):
        sl = slice(i * n_samples, i * n_samples + n_sinkhorn)
        w2.append(W2_distance(samples[sl], target_samples[sl]))
        self_w2.append(W2_distance(target_samples[sl], other_target_samples[sl]))
    return {f"w2_dist{log_prefix}": float(np.mean(w2)), f"w2_dist_std{log_prefix}": float(np.std(w2)),
            f"self_w2_dist{log_prefix}": float(np.mean(self_w2)), f"self_w2_dist_std{log_prefix}": float(np.std(self_w2))}
