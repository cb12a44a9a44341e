"""NumPy float32 restatement of y3_optim_step's update rules, written from the rules, not from the kernel.

Each line is one float32 expression evaluated as written (the library is built with -ffp-contract=off, NumPy never fuses).
D, the decay mask, is a boolean array over the arena; `mask_from_ranges` builds it from [begin, end) pairs and `mask_from_specs`
from a model's spec list (the W segment of every layer; biases, gamma and beta never)."""
import numpy as np

F32 = np.float32
SGD, SGD_NESTEROV, ADAMW = 0, 1, 2
B1, B2, EPS = 0.9, 0.999, 1e-7


def mask_from_ranges(count, ranges):
    d = np.zeros(count, bool)
    for b, e in ranges:
        d[b:e] = True
    return d


def mask_from_specs(specs, count):
    d = np.zeros(count, bool)
    for sp in specs:
        d[sp.w_off:sp.w_off + sp.k * sp.k * sp.cin_pad * sp.cout] = True
    return d


def scaled(g, s=None):
    """g' = g * s with a scale, g without."""
    return g if s is None else g * F32(s)


def sgd_step(p, m, g, lr, mu, wd, D, nesterov=False, s=None):
    """torch.optim.SGD with dampening 0 and coupled L2 -> (p, m)."""
    lr, mu, wd = F32(lr), F32(mu), F32(wd)
    g = scaled(g, s)
    g = np.where(D, g + wd * p, g)
    m = mu * m + g
    u = g + mu * m if nesterov else m
    p = p - lr * u
    assert p.dtype == m.dtype == np.float32
    return p, m


def adamw_step(p, m, v, g, lr_t, lw, D, s=None, b1=B1, b2=B2, eps=EPS):
    """Decoupled decay first, then the Adam step of y3_adam_step (Keras form) -> (p, m, v)."""
    lr_t, lw = F32(lr_t), F32(lw)
    o1, o2 = F32(1) - F32(b1), F32(1) - F32(b2)
    g = scaled(g, s)
    p = np.where(D, p - lw * p, p)
    m = m + (g - m) * o1
    v = v + (g * g - v) * o2
    p = p - (m * lr_t) / (np.sqrt(v) + F32(eps))
    assert p.dtype == m.dtype == v.dtype == np.float32
    return p, m, v


def ema_step(e, x, omd):
    """ema += (x_new - ema) * omd."""
    return e + (x - e) * F32(omd)


def step(kind, p, m, v, g, hyper, D, mu=0.9, wd=0.0, s=None):
    """One step of `kind` with the device pair hyper = (lr or lr_t, lr * wd) -> (p, m, v); v passes through for SGD."""
    if kind == ADAMW:
        return adamw_step(p, m, v, g, hyper[0], hyper[1], D, s)
    p, m = sgd_step(p, m, g, hyper[0], mu, wd, D, kind == SGD_NESTEROV, s)
    return p, m, v


def adamw_hyper(lr, wd, t, b1=B1, b2=B2):
    """{lr_t, lr * wd} of optimiser step t: fp64, rounded once to fp32."""
    return F32(lr * np.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)), F32(lr * wd)
