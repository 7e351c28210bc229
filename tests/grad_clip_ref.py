"""fp64 reference of gradient clipping by global L2 norm followed by AdamW: the norm, the coefficient of
torch.nn.utils.clip_grad_norm_ (norm_type 2, error_if_nonfinite=False) and the AdamW recurrence fed with g * coef.  A helper with
no test of its own: tests/test_grad_clip_host.py vets it against torch in fp64 on the CPU before tests/test_gpu_grad_clip.py lets
it judge the kernels.

The recurrence is written in the kernel's operation order (adamw_kernel, dpft_amd/csrc/optim.hip) and can carry a running
first-order bound on the distance between that fp32 kernel and these fp64 values, 14 roundings per element and step with
u = 2^-24 each (U1 = u / (1 - 16 u) covers the products of roundings), plus the clipped gradient's own error:
  g' = g coef                      E_g  = 3 u |g coef|     (one rounding of the product + the fp32 coefficient's distance from the
                                                            fp64 one, which the norm test bounds by 2 ulp)
  m' = m + (g' - m) c1             E_m' = (1 - c1) E_m + c1 E_g + u (2 |c1 (g' - m)| + |m'|)
  v' = v b2 + (c2 g') g'           E_v' = b2 E_v + 2 c2 |g'| E_g + u (|v b2| + 2 |c2 g' g'| + |v'|)
  s  = sqrt(v')                    E_s  = E_v' / (2 s) + u s          (0 where v' = 0)
  d  = s k + eps                   E_d  = k E_s + u (|s k| + |d|)
  q  = m' / d                      E_q  = E_m' / d + |m'| E_d / d^2 + u |q|
  p' = p decay - step q            E_p' = decay E_p + step E_q + u (|p decay| + |step q| + |p'|)
A contraction of a multiply-add into one fma removes a rounding and never adds one."""
import math

import numpy as np

U = 2.0 ** -24
U1 = U / (1 - 16 * U)


def f32(x):
    return float(np.float32(x))


def sqnorm(grads):
    """Sum of squares in fp64 of a list of arrays (None = no gradient).  Each square of an fp32 value is exact in fp64; the per-
    tensor sums are numpy's pairwise sums and the total is math.fsum of them: good to ~1e-15 relative."""
    return math.fsum(float(np.sum(np.asarray(g, dtype=np.float64) ** 2)) for g in grads if g is not None)


def norm_coef(grads, max_norm):
    """(norm, coef) in fp64: coef = min(1, max_norm / (norm + 1e-6)); a NaN passes through as through torch's clamp.  To judge
    the kernels pass f32(max_norm): the entry point takes max_norm as a float."""
    norm = math.sqrt(sqnorm(grads))
    r = max_norm / (norm + 1e-6)
    return norm, (1.0 if r >= 1.0 else r)


def ulps_f32(got, ref64):
    """Distance of the fp32 value `got` from the fp64 value `ref64` in units of fp32's spacing at ref64."""
    return abs(float(got) - ref64) / float(np.spacing(np.float32(abs(ref64))))


class AdamWRef:
    """AdamW (torch.optim.AdamW: decoupled decay, bias correction, no amsgrad) over a list of fp64 arrays.
    ``kernel_scalars=True``: the hyper-parameters as dpft_adamw_f32 sees them -- fp32 arguments, fp64 arithmetic, fp32
    results (decay, step_size, inv_sqrt_bc2, 1 - beta in fp32); False: everything in fp64, torch's fp64 arithmetic.
    A tensor whose gradient is None sits the step out and keeps its own step count, like torch."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, kernel_scalars=True):
        self.P = [np.asarray(p, dtype=np.float64).copy() for p in params]
        self.M = [np.zeros_like(p) for p in self.P]
        self.V = [np.zeros_like(p) for p in self.P]
        self.EP, self.EM, self.EV = ([np.zeros_like(p) for p in self.P] for _ in range(3))
        self.steps = [0] * len(self.P)
        self.kernel_scalars = kernel_scalars
        if kernel_scalars:
            self.lr, self.b1, self.b2, self.eps, self.wd = f32(lr), f32(betas[0]), f32(betas[1]), f32(eps), f32(weight_decay)
            self.decay = f32(1.0 - self.lr * self.wd)
            self.c1, self.c2 = f32(np.float32(1) - np.float32(betas[0])), f32(np.float32(1) - np.float32(betas[1]))
        else:
            self.lr, self.b1, self.b2, self.eps, self.wd = lr, betas[0], betas[1], eps, weight_decay
            self.decay = 1.0 - lr * weight_decay
            self.c1, self.c2 = 1.0 - betas[0], 1.0 - betas[1]

    def step(self, grads, coef=1.0):
        """One step with the gradients ``grads`` (arrays or None) scaled by ``coef`` (1.0 and no E_g term: unclipped)."""
        for i, g in enumerate(grads):
            if g is None:
                continue
            self.steps[i] += 1
            t = self.steps[i]
            step_size = self.lr / (1.0 - self.b1 ** t)
            k = 1.0 / math.sqrt(1.0 - self.b2 ** t)
            if self.kernel_scalars:
                step_size, k = f32(step_size), f32(k)
            c1, c2, b2, decay, eps = self.c1, self.c2, self.b2, self.decay, self.eps
            gd = np.asarray(g, dtype=np.float64) * coef
            eg = 3 * U1 * np.abs(gd) if coef != 1.0 else np.zeros_like(gd)
            m, v, pp = self.M[i], self.V[i], self.P[i]
            m1 = m + (gd - m) * c1
            em = (1 - c1) * self.EM[i] + c1 * eg + U1 * (2 * np.abs(c1 * (gd - m)) + np.abs(m1))
            v1 = v * b2 + c2 * gd * gd
            ev = b2 * self.EV[i] + 2 * c2 * np.abs(gd) * eg + U1 * (np.abs(v * b2) + 2 * np.abs(c2 * gd * gd) + np.abs(v1))
            s = np.sqrt(v1)
            es = np.where(v1 > 0, ev / (2 * np.where(v1 > 0, s, 1.0)), 0.0) + U1 * s
            d = s * k + eps
            ed = k * es + U1 * (np.abs(s * k) + np.abs(d))
            q = m1 / d
            eq = em / d + np.abs(m1) * ed / d ** 2 + U1 * np.abs(q)
            p1 = pp * decay - step_size * q
            ep = decay * self.EP[i] + step_size * eq + U1 * (np.abs(pp * decay) + np.abs(step_size * q) + np.abs(p1))
            self.M[i], self.V[i], self.P[i], self.EM[i], self.EV[i], self.EP[i] = m1, v1, p1, em, ev, ep

    def clipped_step(self, grads, max_norm):
        """clip_grad_norm_(max_norm) then step(); returns (norm, coef) of the step.  With kernel_scalars max_norm is rounded to
        fp32 first, as every other hyper-parameter is: dpft_grad_clip_coef_f32 takes it as a float."""
        norm, coef = norm_coef(grads, f32(max_norm) if self.kernel_scalars else max_norm)
        self.step(grads, coef)
        return norm, coef
