"""The fused optimiser step of csrc/cgic_adam.hip restated for the tests: torch.optim.Adam's single-tensor chain (torch/optim/adam.py,
the non-capturable branch) with clip_grad_value_ in front and LitEma's update behind it, in numpy fp32 with ONE rounding per operation
(every intermediate is an fp32 array; no fused multiply-add), and the scalar rule of the prologue in Python float64.

The prologue, per entry with a gradient (all float64 unless said):
    step = fp32(step + 1)
    t = the step count as an integer (step_exponent: counts are integers; anything else is cut off, NaN and negatives are 0)
    beta^t by square-and-multiply from the lowest bit of t (power): r = 1, x = beta; while t: if t & 1: r *= x; t >>= 1; if t: x *= x
    step_size = fp32(lr / (1 - beta1^t));  bc2_sqrt = fp32(sqrt(1 - beta2^t))
The body, per element, all fp32:
    g = grad;  clip: g = NaN if g is NaN else -c if g < -c else c if g > c else g;  weight_decay != 0: g = g + wd * p
    w = fp32(1 - beta1):  |w| < 0.5 ?  m = m + w * (g - m)  :  m = g - (g - m) * (1 - w)
    v = v * beta2;  v = v + (fp32(1 - beta2) * g) * g
    p = p + (-step_size) * (m / (sqrt(v) / bc2_sqrt + eps))
    shadow: s = s - (omd * (s - p))   with omd from tests/ema_ref.py
`step64` is the same chain in float64 with exact scalars: what both this restatement and torch's kernels approximate.
"""
import math

import numpy as np

import ema_ref as eref

F = np.float32


def power(beta, t):
    """beta ** t in float64 by square-and-multiply from the lowest bit: a function of (beta, t) alone"""
    r, x, t = 1.0, float(beta), int(t)
    while t:
        if t & 1:
            r = r * x
        t >>= 1
        if t:
            x = x * x
    return r


def step_exponent(step):
    """the fp32 step count as the integer exponent"""
    step = F(step)
    if step >= F(4294967040.0):
        return 4294967040
    return int(step) if step >= F(1.0) else 0


def next_step(step):
    return F(F(step) + F(1.0))


def scalars(step, lr, beta1, beta2):
    """(step_size, bc2_sqrt) as np.float32 for the step count AFTER the increment"""
    t = step_exponent(step)
    bc1, bc2 = 1.0 - power(beta1, t), 1.0 - power(beta2, t)
    with np.errstate(all="ignore"):
        return F(np.float64(lr) / np.float64(bc1)), F(math.sqrt(bc2))


def consts(beta1, beta2, eps, weight_decay, clip_value):
    w1 = F(1.0 - beta1)
    return dict(clip=None if clip_value is None else F(clip_value), wd=F(weight_decay), do_wd=weight_decay != 0, w1=w1, one_minus_w1=F(F(1.0) - w1),
                beta2=F(beta2), w2=F(1.0 - beta2), eps=F(eps), lerp_low=bool(abs(w1) < F(0.5)))


def element(g, p, m, v, k, step_size, bc2_sqrt):
    """one Adam step of fp32 arrays: (p, m, v) afterwards"""
    g, p, m, v = (np.asarray(a, dtype=F) for a in (g, p, m, v))
    step_size, bc2_sqrt = F(step_size), F(bc2_sqrt)
    with np.errstate(all="ignore"):
        if k["clip"] is not None:
            c = k["clip"]
            g = np.where(np.isnan(g), g, np.where(g < -c, -c, np.where(g > c, c, g))).astype(F)
        if k["do_wd"]:
            g = (g + (k["wd"] * p).astype(F)).astype(F)
        diff = (g - m).astype(F)
        if k["lerp_low"]:
            m = (m + (k["w1"] * diff).astype(F)).astype(F)
        else:
            m = (g - (diff * k["one_minus_w1"]).astype(F)).astype(F)
        v = (v * k["beta2"]).astype(F)
        v = (v + ((k["w2"] * g).astype(F) * g).astype(F)).astype(F)
        denom = ((np.sqrt(v).astype(F) / bc2_sqrt).astype(F) + k["eps"]).astype(F)
        p = (p + (F(-step_size) * (m / denom).astype(F)).astype(F)).astype(F)
    return p, m, v


def shadow(s, p, omd):
    s, p, omd = np.asarray(s, dtype=F), np.asarray(p, dtype=F), F(omd)
    with np.errstate(all="ignore"):
        return (s - (omd * (s - p).astype(F)).astype(F)).astype(F)


def step(params, grads, exp_avgs, exp_avg_sqs, steps, lr, betas, eps=1e-8, weight_decay=0.0, clip_value=None, shadows=None, ema_group=None, emas=()):
    """one fused step over lists of fp32 numpy arrays (a gradient or a shadow may be None); steps: fp32 array [entries]; emas: a list of
    [decay, num_updates or None] per EMA group, whose counters move; lr: a float, or an np.float32 for a device tensor's value.
    -> (params, exp_avgs, exp_avg_sqs, steps, shadows) afterwards; emas is updated in place"""
    k = consts(betas[0], betas[1], eps, weight_decay, clip_value)
    n = len(params)
    shadows = list(shadows) if shadows is not None else [None] * n
    ema_group = list(ema_group) if ema_group is not None else [0 if s is not None else -1 for s in shadows]
    omd = []
    for e in emas:
        omd.append(eref.one_minus_decay(e[0], e[1]))
        if e[1] is not None:
            e[1] = eref.next_count(e[1])
    P, M, V, S, T = [], [], [], [], np.array(steps, dtype=F)
    for i in range(n):
        p, m, v, s = params[i], exp_avgs[i], exp_avg_sqs[i], shadows[i]
        if grads[i] is not None:
            T[i] = next_step(T[i])
            step_size, bc2_sqrt = scalars(T[i], float(lr), betas[0], betas[1])
            p, m, v = element(grads[i], p, m, v, k, step_size, bc2_sqrt)
        if s is not None:
            s = shadow(s, p, omd[ema_group[i]])
        P.append(np.array(p, dtype=F)), M.append(np.array(m, dtype=F)), V.append(np.array(v, dtype=F)), S.append(None if s is None else np.array(s, dtype=F))
    return P, M, V, T, S


def step64(p, g, m, v, t, lr, betas, eps=1e-8, weight_decay=0.0, clip_value=None):
    """the same step of ONE tensor in float64 with exact scalars (t: the step number after the increment): (p, m, v) as float64"""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    if clip_value is not None:
        g = np.clip(g, -clip_value, clip_value)
    if weight_decay != 0:
        g = g + weight_decay * p
    m = m + (1.0 - betas[0]) * (g - m)
    v = v * betas[1] + (1.0 - betas[1]) * g * g
    bc1, bc2 = 1.0 - betas[0] ** t, 1.0 - betas[1] ** t
    p = p - (lr / bc1) * (m / (np.sqrt(v) / math.sqrt(bc2) + eps))
    return p, m, v


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=F)).view(np.uint32)


def same_bits(a, b):
    """equal bit for bit, except that a NaN of any payload equals a NaN of any other (ema_ref.same_bits on numpy arrays)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb]))
