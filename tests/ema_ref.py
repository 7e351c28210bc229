"""fp64 reference of the EMA of the weights kept by adamw_kernel<*, true> (dpft_adamw_ema_f32) and by the trainer's eager path:
the one-step rule, the warm-up schedule and the recurrence over a trajectory.  Vetted against torch in tests/test_ema_host.py,
used by tests/test_gpu_ema.py.

The rule is ``ema.lerp_(p, 1 - d)`` (torch.optim.swa_utils.get_ema_multi_avg_fn): e_new = e_old + (p_new - e_old) * w.  The only
fp32 quantity the reference takes over from the kernel is the weight w, formed exactly as the kernel forms it: the decay crosses
the C boundary as a float, d_eff is evaluated in double, and w = (float)(1 - d_eff) is rounded once."""
import numpy as np

U = 2.0 ** -24                                    # unit roundoff of fp32


def decay_eff(decay, warmup=False, own=1):
    """d_eff in double: the fp32-rounded decay, or with warm-up min(decay, (1 + own) / (10 + own)); ``own`` is the tensor's own
    step count, 1 in its first update."""
    d = float(np.float32(decay))
    if warmup:
        d = min(d, (1.0 + float(own)) / (10.0 + float(own)))
    return d


def weight(decay, warmup=False, own=1):
    """w = (float)(1.0 - d_eff), as an np.float32."""
    return np.float32(1.0 - decay_eff(decay, warmup, own))


def one_step(e_old, p_new, w):
    """e_old + (p_new - e_old) * w in fp64, from fp32 (or fp64) inputs and the fp32 weight."""
    e = np.asarray(e_old, dtype=np.float64)
    p = np.asarray(p_new, dtype=np.float64)
    return e + (p - e) * float(w)


def one_step_bound(e_old, p_new):
    """Bound on |fp32 result - one_step()|, per element.  The three fp32 roundings of the kernel (the difference, the product
    -- or none when it is contracted into an fma -- and the sum) give, with |p - e| <= 2 max(|e|, |p|) and |result| <= max(|e|,
    |p|) for 0 <= w <= 1, at most (4 w + 1) u max(|e|, |p|) to first order; 4 * 2^-23 max(|e|, |p|) = 8 u max is that with a
    factor below 2 of slack."""
    m = np.maximum(np.abs(np.asarray(e_old, dtype=np.float64)), np.abs(np.asarray(p_new, dtype=np.float64)))
    return 4.0 * 2.0 ** -23 * m


def trajectory(e0, ps, ws):
    """The recurrence over a trajectory: e_0 = e0, e_{k+1} = one_step(e_k, ps[k], ws[k]); ws[k] None = the tensor sits step k
    out.  Returns the list [e_1, ..., e_K] (fp64)."""
    e = np.asarray(e0, dtype=np.float64)
    out = []
    for p, w in zip(ps, ws):
        if w is not None:
            e = one_step(e, p, w)
        out.append(e)
    return out
