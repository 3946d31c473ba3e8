"""Command-line driver with the reference's flag surface: `python -m cmcd_amd.main --config.model many_gmm
--config.boundmode MCD_CAIS_sn --config.N 2000 --config.nbridges 256 --noconfig.pretrain_mfvi ...` runs what
`python main.py --config.model ...` runs in /root/reference/src (main.py:52-300), on the HIP path:

  mean-field pre-training (config.pretrain_mfvi)  ->  mcdbm.initialize(vdparams=vdparams_init)  ->  opt.run
  ->  opt.sample / log_final_losses (n_input_dist_seeds x n_samples)  [-> the same with the EMA parameters]

Flag names, defaults and the `--config.x value` / `--config.x=value` / `--noconfig.x` forms follow
/root/reference/src/configs/base.py:77-155 (ml_collections + absl).  Left out: W&B, plotting, the inference-gym rows of the lr table.  `UHA` (Hamiltonian AIS, the reference's default
boundmode) runs through cmcd_amd.hais (lgcp: cmcd_amd.hais_lgcp) on one GPU; modes outside it, the overdamped family and 2nd-order CMCD (`MCD_CAIS_UHA_sn`)
raise NotImplementedError exactly like the library.  Under torchrun the particles of every iteration are sharded over the
ranks (parallel.make_sharded_grad_and_loss)."""
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def get_config():
    """/root/reference/src/configs/base.py:77-155 (the fields this driver reads)."""
    c = types.SimpleNamespace()
    c.boundmode = "UHA"
    c.model = "lorenz"
    c.N = 5
    c.nbridges = 8
    c.lfsteps = 1
    c.emb_dim = 20
    c.nlayers = 3
    c.init_eta = 0.0
    c.init_eps = 1e-5
    c.init_sigma = 1.0
    c.pretrain_mfvi = True
    c.train_vi = True
    c.train_eps = True
    c.train_betas = True
    c.nn_arch = "geffner"
    c.eps_schedule = ""
    c.grad_clipping = False
    c.mfvi_iters = 150000
    c.mfvi_lr = 0.01
    c.iters = 150000
    c.lr = 0.0001
    c.seed = 1
    c.n_samples = 500
    c.n_input_dist_seeds = 30
    c.n_sinkhorn = 300      # read by nobody, like the reference (main.py passes n_samples)
    c.use_ema = False
    c.funnel_sig = 3
    c.funnel_clipy = 11
    c.funnel_d = 10
    c.n_mixes = 40
    c.loc_scaling = 40
    c.file_path = os.path.join(os.getcwd(), "../pines.csv")
    c.save_params = ""          # extra: path of a params.pkl to write (the reference logs it as a W&B artifact)
    c.init_gamma = 10.0         # extra: the reference has no such flag — mcdbm.initialize's default gamma = 10.0 is what
    #                             its main.py always uses (main.py:148-159); only MCD_CAIS_UHA_sn reads gamma
    c.compute_w2 = True         # extra: --noconfig.compute_w2 skips the Sinkhorn W2 block of main.py:248-271 (test harness)
    c.compute_eubo = True       # extra: --noconfig.compute_eubo skips the reverse-chain diagnostics (EUBO, reverse ln Z / ESS)
    c.eubo_uha = False          # extra: --config.eubo_uha adds the reverse-chain line to boundmode UHA (cmcd_amd.reverse_hais).  Off by
    #                             default, unlike the MCD modes: tests/test_gpu_hais.py::test_driver_runs_the_default_boundmode holds
    #                             the default UHA command line to printing no "Reverse chain" line, and existing tests stay as they are
    c.smc_eval = False         # extra: --config.smc_eval adds the SMC evaluation (cmcd_amd.smc / smc_uha / smc_ldvi / smc_hais: resampling between bridges)
    # fields of the reference's config this driver accepts so that its README command lines run unchanged, but whose
    # only legal value here is the default (dds nets are 64-wide, the lgcp posterior is un-whitened, 40 mixtures
    # unless n_mixes says otherwise) or that configure subsystems left out (NICE, W&B, the cluster launcher)
    c.fully_connected_units = "[64, 64]"
    c.use_whitened = False
    c.gmm_easy_mode = False
    c.id = -1
    c.run_cluster = 0
    c.im_size, c.alpha, c.n_bits, c.hidden_dim = 14, 0.05, 3, 1000
    c.wandb = types.SimpleNamespace(log=True, project="final_cmcd", entity="shreyaspadhy", code_dir=os.getcwd(),
                                    name="", log_artifact=True)
    return c


# /root/reference/src/configs/base.py:5-75 (the entries of the models this build runs)
LR_DICT = {"lgcp": {"MCD_CAIS_UHA_sn": 1e-3, "MCD_CAIS_sn": 1e-4, "MCD_U_a-lp-sn": 1e-3, "UHA": 1e-4, "MCD_ULA_sn": 1e-4,
                    "MCD_ULA": 1e-4}}
FUNNEL_EPS_DICT = {8: {"init_eps": 0.1, "lr": 0.01}, 16: {"init_eps": 0.1, "lr": 0.01}, 32: {"init_eps": 0.1, "lr": 0.005},
                   64: {"init_eps": 0.1, "lr": 0.001}, 128: {"init_eps": 0.01, "lr": 0.01}, 256: {"init_eps": 0.01, "lr": 0.005}}


def setup_config(config):
    """/root/reference/src/utils.py:181-204: the tuned lr / init_eps that main.py writes over the flags
    (funnel: by nbridges; lgcp: by boundmode; gmm / many_gmm: none; unknown keys: none)."""
    try:
        if config.model == "funnel":
            config.init_eps, config.lr = FUNNEL_EPS_DICT[config.nbridges]["init_eps"], FUNNEL_EPS_DICT[config.nbridges]["lr"]
        elif config.model not in ("many_gmm", "gmm"):
            config.lr = LR_DICT[config.model][config.boundmode]
    except KeyError:
        print("LR not found for model %s and boundmode %s" % (config.model, config.boundmode))
    return config


def _field(config, dotted):
    """`wandb.name` -> (config.wandb, "name")"""
    node, parts = config, dotted.split(".")
    for part in parts[:-1]:
        node = getattr(node, part, None)
        if not isinstance(node, types.SimpleNamespace):
            raise SystemExit(f"unknown config field {dotted!r}")
    if not hasattr(node, parts[-1]) or isinstance(getattr(node, parts[-1]), types.SimpleNamespace):
        raise SystemExit(f"unknown config field {dotted!r}")
    return node, parts[-1]


def parse_flags(argv, config):
    """absl / ml_collections style: --config.name value | --config.name=value | --config.flag | --noconfig.flag
    (absl also takes a single leading dash; the reference's README uses it once)."""
    i = 0
    while i < len(argv):
        a = argv[i]
        if a.startswith("-") and not a.startswith("--"):
            a = "-" + a
        if a.startswith("--noconfig."):
            node, name = _field(config, a[len("--noconfig."):])
            if not isinstance(getattr(node, name), bool):
                raise SystemExit(f"{a}: not a boolean field")
            setattr(node, name, False)
            i += 1
            continue
        if not a.startswith("--config."):
            raise SystemExit(f"unknown argument {a!r} (expected --config.<field> ...)")
        dotted, eq, val = a[len("--config."):].partition("=")
        node, name = _field(config, dotted)
        cur = getattr(node, name)
        if isinstance(cur, bool):
            if eq:
                setattr(node, name, val.lower() in ("1", "true", "yes"))
            else:
                setattr(node, name, True)
            i += 1
            continue
        if not eq:
            i += 1
            if i >= len(argv):
                raise SystemExit(f"--config.{dotted} needs a value")
            val = argv[i]
        setattr(node, name, type(cur)(val) if not isinstance(cur, str) else val)
        i += 1
    return config


def check_fixed_fields(config):
    """The accepted-but-fixed fields: fail loudly rather than silently run something else."""
    units = [int(u) for u in str(config.fully_connected_units).strip("[]() ").replace(" ", "").split(",") if u]
    if config.nn_arch in ("dds", "dds_grad") and units != [64, 64]:
        raise NotImplementedError(f"fully_connected_units={units}: the HIP path builds the dds net 64 wide")
    if config.use_whitened:
        raise NotImplementedError("use_whitened=True: the lgcp kernels evaluate the un-whitened posterior")
    # gmm_easy_mode is read once while the reference builds its defaults (configs/base.py:137-143), so the flag changes
    # nothing there either; wandb.* configure a logger this build replaces by stdout


def main(config):
    import torch.distributed as dist
    from . import boundingmachine as bm
    from . import mcdboundingmachine as mcdbm
    from . import _chain, opt, parallel, resample, utils
    from .model_handler import load_model

    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("cmcd_amd.main needs a ROCm GPU (no CPU fallback for the hot path)")
    torch.cuda.set_device(local)
    if "RANK" in os.environ and "MASTER_PORT" in os.environ:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    say = print if rank == 0 else (lambda *a, **k: None)
    setup_config(config)                                                   # main.py:64-66
    check_fixed_fields(config)
    say({k: v for k, v in vars(config).items() if k != "wandb"})

    if "lgcp" in config.model and not os.path.exists(config.file_path):
        # the point set is reference content; its 40 x 40 bin counts ship as a test fixture
        from .lgcp import load_model_lgcp
        counts = np.load(os.path.join(ROOT, "tests", "golden", "lgcp_bin_counts.npy"))
        res = load_model_lgcp(config.model, config, flat_bin_counts=counts)
    else:
        res = load_model(config.model, config)
    log_prob_model, dim = res[0], res[1]
    sample_from_target_fn = res[2] if len(res) > 2 and config.model in ("funnel", "gmm", "many_gmm") else None   # TRACTABLE_DISTS

    gen = torch.Generator().manual_seed(config.seed)                       # train_rng_key_gen
    eval_gen = torch.Generator().manual_seed(config.seed + 1)              # eval_rng_key_gen
    device = torch.device("cuda", local)

    # Train initial variational distribution to maximize the ELBO            main.py:81-109
    trainable = ("vd",)
    params_flat, unflatten, params_fixed = bm.initialize(dim=dim, nbridges=0, trainable=trainable,
                                                         init_sigma=config.init_sigma, device=device)
    if config.pretrain_mfvi:
        losses, params_flat, _ = opt.run(config, config.mfvi_lr, config.mfvi_iters, params_flat, unflatten, params_fixed,
                                         log_prob_model, bm.grad_and_loss, trainable, gen, log_prefix="pretrain")
        elbo_init = -float(np.mean(losses[-500:]))
        say("Done training initial parameters, got ELBO %.2f." % elbo_init)
    vdparams_init = {k: v.detach().cpu().clone() for k, v in unflatten(params_flat)[0]["vd"].items()}

    if config.boundmode == "UHA":                                          # main.py:115-136
        # Hamiltonian AIS (cmcd_amd.hais; lgcp: cmcd_amd.hais_lgcp).  The reference writes `trainable = "eta"`, a str, and its `trainable + ("eps",)` raises
        # TypeError with its own default flags; the tuple below is what it means.
        if config.model == "lgcp":      # d = 1600: the launch sequence of cmcd_amd.hais_lgcp, same interface
            from . import hais_lgcp as hais
        else:
            from . import hais
        if world > 1:
            raise NotImplementedError("boundmode UHA runs on one GPU: its particles are not sharded over ranks")
        trainable = ("eta",)
        if config.train_eps:
            trainable += ("eps",)
        if config.train_vi:
            trainable += ("vd",)
        if config.train_betas:
            trainable += ("mgridref_y",)
        say(f"Params being trained : {trainable}")
        params_flat, unflatten, params_fixed = hais.initialize(
            dim=dim, nbridges=config.nbridges, eta=config.init_eta, eps=config.init_eps, lfsteps=config.lfsteps,
            vdparams=vdparams_init, trainable=trainable, device=device)
        grad_and_loss, loss_fn = hais.grad_and_loss, hais.compute_bound
    elif config.boundmode in ("MCD_U_a-lp-sn", "MCD_U_a-lp"):             # LDVI and its network-free sibling (cmcd_amd.ldvi)
        from . import ldvi
        if world > 1:
            raise NotImplementedError("boundmode %s runs on one GPU: its particles are not sharded over ranks" % config.boundmode)
        trainable = ("eta", "gamma")                                       # main.py:137-146 (eta is not read by this mode)
        if config.train_eps:
            trainable += ("eps",)
        if config.train_vi:
            trainable += ("vd",)
        if config.train_betas:
            trainable += ("mgridref_y",)
        say(f"Params being trained : {trainable}")
        params_flat, unflatten, params_fixed = ldvi.initialize(
            dim=dim, nbridges=config.nbridges, vdparams=vdparams_init, eta=config.init_eta, eps=config.init_eps,
            gamma=config.init_gamma, trainable=trainable, mode=config.boundmode, emb_dim=config.emb_dim, nlayers=config.nlayers,
            nn_arch=config.nn_arch, device=device)
        grad_and_loss, loss_fn = ldvi.grad_and_loss, ldvi.compute_bound
    elif "MCD" in config.boundmode:
        trainable = ("eta", "gamma")
        if config.train_eps:
            trainable += ("eps",)
        if config.train_vi:
            trainable += ("vd",)
        if config.train_betas:
            trainable += ("mgridref_y",)
        say(f"Params being trained : {trainable}")
        params_flat, unflatten, params_fixed = mcdbm.initialize(
            dim=dim, nbridges=config.nbridges, vdparams=vdparams_init, eta=config.init_eta, eps=config.init_eps,
            gamma=config.init_gamma, trainable=trainable, mode=config.boundmode, emb_dim=config.emb_dim, nlayers=config.nlayers,
            nn_arch=config.nn_arch, device=device)
        grad_and_loss, loss_fn = mcdbm.make_grad_and_loss(config.boundmode, eps_schedule=config.eps_schedule,
                                                          grad_clipping=config.grad_clipping)
        if world > 1:
            grad_and_loss = parallel.make_sharded_grad_and_loss(config.boundmode, eps_schedule=config.eps_schedule,
                                                                grad_clipping=config.grad_clipping)
    else:
        raise NotImplementedError("Mode %s not implemented." % config.boundmode)

    t0 = time.time()
    _, params_flat, ema_params = opt.run(config, config.lr, config.iters, params_flat, unflatten, params_fixed,
                                         log_prob_model, grad_and_loss, trainable, gen, use_ema=config.use_ema)
    torch.cuda.synchronize()
    say("%d iterations in %.1f s" % (config.iters, time.time() - t0))

    # Average over n_input_dist_seeds seeds, n_samples samples each, after training is done.   main.py:179-226
    n = config.n_samples * config.n_input_dist_seeds
    eval_seeds = torch.randint(1, 1000000, (n,), generator=eval_gen, dtype=torch.int32).to(device)
    eval_losses, samples = utils.sample(config, config.n_samples, config.n_input_dist_seeds, params_flat, unflatten,
                                        params_fixed, log_prob_model, loss_fn, eval_seeds, log_prefix="eval")
    final_elbo, final_ln_Z = utils.log_final_losses(eval_losses.cpu())
    say("Done training, got ELBO %.2f." % final_elbo)
    say("Done training, got ln Z %.2f." % final_ln_Z)
    ess = utils.log_importance_diagnostics(eval_losses)
    say("Importance weights behind ln Z: ESS %.1f (+- %.1f) of %d samples per group (%.1f %%)." % (
        ess["ess"], ess["ess_std"], config.n_samples, 100.0 * ess["ess_frac"]))
    # The other half of the diagnostics (no analogue in the reference): exact target draws through the backward kernels.
    # (MCD_CAIS_UHA_sn: the chain carries a momentum, cmcd_amd.reverse_uha; same line, same diagnostics on w)
    # (LDVI: cmcd_amd.reverse_ldvi.  UHA: cmcd_amd.reverse_hais, behind --config.eubo_uha only: the default UHA command line is
    # held by tests/test_gpu_hais.py::test_driver_runs_the_default_boundmode to print no such line)
    reverse = (config.compute_eubo and sample_from_target_fn is not None and rank == 0 and
               (config.boundmode in ("MCD_CAIS_sn", "MCD_CAIS_var_sn", "MCD_ULA", "MCD_ULA_sn", "MCD_CAIS_UHA_sn",
                                     "MCD_U_a-lp-sn", "MCD_U_a-lp") or (config.boundmode == "UHA" and config.eubo_uha)))
    if reverse:
        from .model_handler import exact_target_draws
        rev = _chain.reverse_module(config.boundmode)
        x_tgt = torch.from_numpy(exact_target_draws(config.model, sample_from_target_fn, 3, n, dim)).to(device)   # (seeds 1, 2: the W2 block)

        def say_reverse(p, forward_elbo, forward_ln_Z, prefix=""):
            w = rev.bound_reverse(eval_seeds, x_tgt, p, unflatten, params_fixed, log_prob_model,
                                  eps_schedule=config.eps_schedule, grad_clipping=config.grad_clipping)[0]
            r = utils.log_reverse_diagnostics(w.view(config.n_input_dist_seeds, config.n_samples), log_prefix=prefix)
            say("Reverse chain%s: EUBO %.2f, reverse ln Z %.2f, reverse ESS %.1f (+- %.1f) of %d (%.1f %%); ln Z bracket "
                "[ELBO %.2f, EUBO %.2f], forward ln Z %.2f." % (
                    prefix, r["eubo" + prefix], r["reverse_ln_Z" + prefix], r["reverse_ess" + prefix],
                    r["reverse_ess_std" + prefix], config.n_samples, 100.0 * r["reverse_ess_frac" + prefix], forward_elbo,
                    r["eubo" + prefix], forward_ln_Z))

        say_reverse(params_flat, final_elbo, final_ln_Z)
    # SMC evaluation (no analogue in the reference): the same chain with the groups resampled between bridges when their ESS drops
    # (the three momentum modes carry rho in the state: MCD_CAIS_UHA_sn cmcd_amd.smc_uha, LDVI cmcd_amd.smc_ldvi, UHA
    # cmcd_amd.smc_hais; same driver, same result dict.  UHA on lgcp has no segments: cmcd_amd.hais_lgcp runs whole chains)
    smc_on = (config.smc_eval and rank == 0 and config.model in ("funnel", "gmm", "many_gmm") and
              (config.boundmode in ("MCD_CAIS_sn", "MCD_CAIS_var_sn", "MCD_ULA", "MCD_ULA_sn", "MCD_CAIS_UHA_sn", "MCD_U_a-lp-sn",
                                    "MCD_U_a-lp") or (config.boundmode == "UHA" and config.nbridges >= 1)))
    if smc_on:
        from . import sinkhorn
        smc = _chain.smc_module(config.boundmode)

        def say_smc(p, prefix=""):
            G = config.n_input_dist_seeds
            res = smc.smc_bound(eval_seeds, p, unflatten, params_fixed, log_prob_model, eps_schedule=config.eps_schedule,
                                grad_clipping=config.grad_clipping, groups=G, seed=config.seed)
            r = utils.log_smc_diagnostics(res, log_prefix=prefix)
            line = "SMC%s: ln Z %.2f (+- %.2f), %d resampling events in %d stages, final ESS %.1f (+- %.1f) of %d (%.1f %%)" % (
                prefix, r["smc_ln_Z" + prefix], r["smc_ln_Z_std" + prefix], r["smc_resampling_events" + prefix],
                r["smc_stages" + prefix], r["smc_ess" + prefix], r["smc_ess_std" + prefix], config.n_samples,
                100.0 * r["smc_ess_frac" + prefix])
            if sample_from_target_fn is not None and config.compute_w2:
                cloud, _, _ = resample.resample(res["losses"], res["z"], groups=G, seed=config.seed)
                draws = sample_from_target_fn(1, (n,)) if config.model == "many_gmm" else sample_from_target_fn(1, n)
                tgt_smc = torch.from_numpy(np.ascontiguousarray(draws, dtype=np.float32)).to(device)
                cost = sinkhorn.w2_batched(cloud.view(G, config.n_samples, dim), tgt_smc.view(G, config.n_samples, dim))["cost"]
                line += "; W2 of the resampled SMC cloud to the target %.4f (+- %.4f)" % (
                    float(cost.mean()), float(cost.std(unbiased=False)))
            say(line + ".")

        say_smc(params_flat)
    if config.use_ema:
        eval_losses_ema, samples_ema = utils.sample(config, config.n_samples, config.n_input_dist_seeds, ema_params, unflatten,
                                          params_fixed, log_prob_model, loss_fn, eval_seeds, log_prefix="eval")
        e2, z2 = utils.log_final_losses(eval_losses_ema.cpu(), log_prefix="_ema")
        say("With EMA, got ELBO %.2f." % e2)
        say("With EMA, got ln Z %.2f." % z2)
        if reverse:
            say_reverse(ema_params, e2, z2, prefix="_ema")
        if smc_on:
            say_smc(ema_params, prefix="_ema")
    if sample_from_target_fn is not None and config.model in ("funnel", "gmm") and rank == 0 and config.compute_w2:   # main.py:248-271
        tgt = torch.from_numpy(sample_from_target_fn(1, n)).to(device)
        other = torch.from_numpy(sample_from_target_fn(2, n)).to(device)
        clouds = [("", samples)] + ([("_ema", samples_ema)] if config.use_ema else [])
        self_w2 = None
        for prefix, cloud in clouds:
            # one batched solve (cmcd_amd.sinkhorn) per cloud: the cloud as it is, the same cloud importance-resampled within
            # each seed group (weights exp(-loss), systematic scheme), the cloud weighted by softmax(-loss), and — once —
            # the two target draws against each other
            cloud_losses = eval_losses_ema if prefix else eval_losses
            resampled, _, _ = resample.resample(cloud_losses, cloud, groups=config.n_input_dist_seeds, seed=config.seed)
            w2 = utils.calculate_W2_distances(cloud, tgt, other, config.n_samples, config.n_input_dist_seeds,
                                              config.n_samples, log_prefix=prefix, losses=cloud_losses,
                                              also={"resampled": resampled}, self_w2=self_w2)
            self_w2 = (w2["self_w2_dist" + prefix], w2["self_w2_dist_std" + prefix])
            say("W2%s to the target %.4f (+- %.4f); between two target draws %.4f (+- %.4f)" % (
                prefix, w2["w2_dist" + prefix], w2["w2_dist_std" + prefix], w2["self_w2_dist" + prefix],
                w2["self_w2_dist_std" + prefix]))
            say("W2%s of the resampled cloud to the target %.4f (+- %.4f)" % (
                prefix, w2["w2_dist_resampled" + prefix], w2["w2_dist_resampled_std" + prefix]))
            say("W2%s of the weighted cloud to the target %.4f (+- %.4f)" % (
                prefix, w2["w2_weighted_dist" + prefix], w2["w2_weighted_dist_std" + prefix]))
    if config.save_params and rank == 0:
        utils.save_params(config.save_params, params_flat, unflatten)
    if dist.is_initialized():
        dist.destroy_process_group()
    return final_elbo, final_ln_Z


if __name__ == "__main__":
    main(parse_flags(sys.argv[1:], get_config()))
