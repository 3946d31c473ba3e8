"""The optimiser step of the reference's training loop, restated in NumPy with optax's definitions: the yardstick of
tests/test_oracle_opt.py and tests/test_gpu_opt.py for `adam_step_kernel` (cmcd_amd/csrc/cmcd_opt.hip).

One call of `step` is the loop body of /root/reference/src/opt.py:14-35, 122-134:

  1. g = clip(grad, +-clip)            optax.clip = jnp.clip: NaN passes through, +-inf is clipped
  2. mu = b1 mu + (1 - b1) g,  nu = b2 nu + (1 - b2) g^2          optax.scale_by_adam: moments of the clipped gradient
  3. p -= lr (mu / (1 - b1^t)) / (sqrt(nu / (1 - b2^t)) + eps)    bias correction, eps outside the root
  4. the projection ranges, in order: clamp min(max(x, lo), hi) or relu floor max(x - lo, 0) + lo; both propagate NaN
  5. ema = (1 - s) ema + s p           optax.incremental_update
  6. with `losses`: the step is skipped when mean(losses) is NaN (a NaN loss, or +inf and -inf both) or `flag != 0`;
     a skipped step leaves all four arrays untouched and sets the flag.

The hyperparameters are the float32 values the C ABI receives, taken exactly into float64; `1 - b` is `1 - float32(b)`,
which float32 represents exactly for b = 0.9 and b = 0.999.  `dtype=np.float32` runs the same operation order in float32:
that is the measurement of the float32 gap, not a yardstick.

`one_minus`:
  "float32" (default)  1 - float32(b), as above.
  "optax"              optax's own float32 constant for 1 - b2: the Python double 1 - 0.999 rounded to float32, which is
                       1.0000128 x (1 - float32(0.999)).  For the one test that records this distance; nothing else uses it.
  "python"             every hyperparameter, 1 - b and the range bounds as Python doubles, unrounded: the constants of the eager CPU path
                       (opt._ClipAdam.update), for the one comparison with that path.
"""
import numpy as np

CLAMP, RELU_FLOOR = 0, 1
HYPER = dict(lr=0.01, b1=0.9, b2=0.999, eps=1e-8, clip=5.0, ema_step=0.001)


def f32(x):
    """The float32 value the C ABI receives for a Python double, as a Python double."""
    return float(np.float32(x))


def mean_is_nan(losses):
    """Whether jnp.mean(losses) is NaN: a NaN loss, or +inf and -inf both.  (A float32 sum that merely overflows gives
    +-inf, not NaN: the step goes through.)"""
    l = np.asarray(losses, np.float64)
    return bool(np.isnan(l).any() or ((l == np.inf).any() and (l == -np.inf).any()))


def project(p, ranges, dtype=np.float64, exact_bounds=False):
    """The ranges (offset, length, kind, lo, hi), applied in order, in place on `p`; lo / hi are taken as the float32 values
    of the C record (`exact_bounds`: as the Python doubles given)."""
    for off, length, kind, lo, hi in ranges:
        if length <= 0:
            continue
        x = p[off:off + length]
        lo_, hi_ = (dtype(lo), dtype(hi)) if exact_bounds else (dtype(np.float32(lo)), dtype(np.float32(hi)))
        with np.errstate(invalid="ignore"):
            if kind == CLAMP:
                x[...] = np.minimum(np.maximum(x, lo_), hi_)          # np.maximum / np.minimum propagate NaN, as jnp.clip
            else:
                x[...] = np.maximum(x - lo_, dtype(0)) + lo_          # jax.nn.relu(x - lo) + lo
    return p


def step(state, grad, hyper, t, ranges=(), losses=None, flag=0, dtype=np.float64, one_minus="float32"):
    """-> (params, mu, nu, ema, flag, skipped).  `state` = (params, mu, nu, ema) with ema possibly None; the inputs are not
    modified.  `hyper`: dict with lr, b1, b2, eps, clip, ema_step (missing keys from HYPER).  `t` >= 1: the step's count."""
    assert one_minus in ("float32", "optax", "python") and t >= 1
    h = dict(HYPER)
    h.update(hyper or {})
    conv = float if one_minus == "python" else f32
    lr, b1, b2, eps, clip, s = (conv(h[k]) for k in ("lr", "b1", "b2", "eps", "clip", "ema_step"))
    omb1, omb2 = 1.0 - b1, 1.0 - b2
    if one_minus == "optax":
        omb2 = f32(1.0 - float(h["b2"]))
    p, mu, nu, ema = (None if a is None else np.array(a, dtype=dtype) for a in state)
    if losses is not None and (mean_is_nan(losses) or flag != 0):
        return p, mu, nu, ema, 1, True
    d = dtype
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        g = np.clip(np.array(grad, dtype=d), d(-clip), d(clip))
        mu = d(b1) * mu + d(omb1) * g
        nu = d(b2) * nu + d(omb2) * g * g
        if d is np.float64:
            b1t, b2t = (b1 ** t if b1 > 0 else 0.0), b2 ** t           # Python doubles: underflow to 0 for huge t
        else:
            b1t, b2t = np.power(d(b1), d(t)), np.power(d(b2), d(t))
        mu_hat = mu / (d(1) - d(b1t))
        nu_hat = nu / (d(1) - d(b2t))
        p = p - d(lr) * mu_hat / (np.sqrt(nu_hat) + d(eps))
        project(p, ranges, d, exact_bounds=one_minus == "python")
        if ema is not None:
            ema = (d(1) - d(s)) * ema + d(s) * p
    return p, mu, nu, ema, flag, False
