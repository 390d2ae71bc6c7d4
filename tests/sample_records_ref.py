"""float32 numpy reference of the frame path's sample records: what the consumers of (t, ray id) rebuild.

Every operation is one IEEE binary32 operation in the written order (the contract at the top of oracle/march.py):

    p     = clamp(o + t*d, -bound, bound)               position (mul, add, clamp)
    x01   = (p + bound) * (1 / (2 bound))               field kernel; == (p + bound) / (2 bound) for a power-of-two 2*bound
    dt    = clamp(t*dt_gamma, dt_min, dt_max)
    tn    = t + dt;  delta = tn - last_t;  last_t = tn  compositing; last_t starts at t0 = near + dt(near) * noise
"""
import numpy as np

F32 = np.float32
SQRT3_2 = F32(3.4641016151377544)   # float32(2*sqrt(3))


def dt_limits(max_steps, cascade, H):
    return F32(SQRT3_2 / F32(max_steps)), F32(SQRT3_2 * F32(2 ** (cascade - 1)) / F32(H))


def step_dt(t, dt_gamma, max_steps, cascade, H):
    lo, hi = dt_limits(max_steps, cascade, H)
    return np.minimum(np.maximum(np.asarray(t, F32) * F32(dt_gamma), lo), hi).astype(F32)


def start_t(nears, noises, dt_gamma, max_steps, cascade, H):
    nears = np.asarray(nears, F32)
    noises = np.zeros_like(nears) if noises is None else np.asarray(noises, F32)
    return (nears + step_dt(nears, dt_gamma, max_steps, cascade, H) * noises).astype(F32)


def position(o, d, t, bound):
    """o, d [..., 3], t [...] -> p [..., 3]"""
    b = F32(bound)
    prod = (np.asarray(t, F32)[..., None] * np.asarray(d, F32)).astype(F32)
    return np.minimum(np.maximum((np.asarray(o, F32) + prod).astype(F32), -b), b).astype(F32)


def x01_div(p, bound):
    return ((np.asarray(p, F32) + F32(bound)).astype(F32) / F32(2.0 * bound)).astype(F32)


def x01_mul(p, bound):
    return ((np.asarray(p, F32) + F32(bound)).astype(F32) * (F32(1.0) / F32(2.0 * bound))).astype(F32)


def deltas_of_ray(t, t0, dt_gamma, max_steps, cascade, H):
    """t [k]: the ray's samples in order, t0 its start -> deltas [k,2] = (dt, tn - last_t)."""
    t = np.asarray(t, F32)
    dt = step_dt(t, dt_gamma, max_steps, cascade, H)
    tn = (t + dt).astype(F32)
    last = np.concatenate([np.asarray([t0], F32), tn[:-1]])
    return np.stack([dt, (tn - last).astype(F32)], -1)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, F32)).view(np.uint32)
