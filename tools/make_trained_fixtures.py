"""Generates tests/golden/trained_<id>.npz: run once on the MI355X.

Every row of tests/trained_cases.TRAINED_ROWS is trained by the project's own loop — `opt.run` on
`mcdbm.make_grad_and_loss(boundmode, ...)`, `hais.grad_and_loss` for boundmode UHA — from the start `cmcd_amd.main` gives it
(no mean-field pre-training: the rows' `--noconfig.pretrain_mfvi`), with the row's flags, and the final merged `params` dict
(utils.params_to_numpy, float32) is stored with those flags.  The files are INPUTS of tests/test_oracle_trained_params.py and
tests/test_gpu_trained.py, produced by the code under test; every expected value there comes from the float64 oracle.

  python tools/make_trained_fixtures.py [id ...] [--set flag=value ...]

(`--set` tries a row with other flags, e.g. `--set lr=0.001 --set iters=1000`: the file records what ran, and the tests refuse
it until TRAINED_ROWS lists the same) prints, per row, the time of the run and the mean loss at its start and end, and how far each trainable leaf moved.
"""
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from cmcd_amd import hais, opt, utils  # noqa: E402
from cmcd_amd import mcdboundingmachine as mcdbm  # noqa: E402
from cmcd_amd import variationaldist as vd  # noqa: E402
from cmcd_amd.model_handler import load_model  # noqa: E402
import trained_cases as tc  # noqa: E402


def train(cid, row):
    info = types.SimpleNamespace(**row)
    target, dim = load_model(row["model"], info)[:2]
    trainable = tc.trainable_of(row)
    vdparams = vd.initialize(dim, init_sigma=row["init_sigma"])
    if row["boundmode"] == "UHA":
        flat, un, fixed = hais.initialize(dim=dim, nbridges=row["nbridges"], eta=row["init_eta"], eps=row["init_eps"],
                                          lfsteps=row["lfsteps"], vdparams=vdparams, trainable=trainable, device="cuda")
        grad_and_loss = hais.grad_and_loss
    else:
        flat, un, fixed = mcdbm.initialize(dim=dim, nbridges=row["nbridges"], vdparams=vdparams, eta=0.0, eps=row["init_eps"],
                                           gamma=row.get("init_gamma", 10.0), trainable=trainable, mode=row["boundmode"],
                                           emb_dim=row["emb_dim"], nlayers=3, nn_arch=row["nn_arch"], device="cuda")
        grad_and_loss, _ = mcdbm.make_grad_and_loss(row["boundmode"], eps_schedule=row["eps_schedule"],
                                                    grad_clipping=row["grad_clipping"])
    t0 = time.time()
    losses, out, _ = opt.run(info, row["lr"], row["iters"], flat, un, fixed, target, grad_and_loss, trainable,
                             torch.Generator().manual_seed(row["seed"]))
    torch.cuda.synchronize()
    dt = time.time() - t0
    assert bool(torch.isfinite(out).all()), f"{cid}: non-finite parameters after {len(losses)} logged losses, last {losses[-3:]}"
    first, last = float(np.mean(losses[:10])), float(np.mean(losses[-10:]))
    print(f"{cid}: {row['iters']} iterations in {dt:.1f} s ({1e3 * dt / row['iters']:.3f} ms each), {len(losses)} logged; "
          f"mean loss {first:.4f} -> {last:.4f}", flush=True)
    a, b = flat.cpu(), out.cpu()
    for path, (off, shape) in un.layout.items():
        n = max(1, int(np.prod(shape)))
        print("   ", "train  " if path[0] == 0 else "notrain", "/".join(map(str, path[1:])), tuple(shape),
              "max |change| %.3e" % float((a[off:off + n] - b[off:off + n]).abs().max()),
              "max |value| %.3e" % float(b[off:off + n].abs().max()))
    made_by = (f"tools/make_trained_fixtures.py on {torch.cuda.get_device_name(0)}: opt.run, {row['iters']} iterations, "
               f"trainable {trainable}, final mean loss {last:.6f}")
    path = tc.fixture_path(cid)
    tc.save_fixture(path, row, utils.params_to_numpy(out, un), made_by)
    print("    wrote", os.path.relpath(path, ROOT), os.path.getsize(path), "bytes", flush=True)


def main():
    args, over = sys.argv[1:], {}
    while "--set" in args:
        i = args.index("--set")
        key, val = args[i + 1].split("=", 1)
        over[key] = type(tc._GMM[key])(val)
        del args[i:i + 2]
    os.makedirs(tc.GOLD, exist_ok=True)
    for cid in args or list(tc.TRAINED_ROWS):
        train(cid, dict(tc.TRAINED_ROWS[cid], **over))


if __name__ == "__main__":
    main()
