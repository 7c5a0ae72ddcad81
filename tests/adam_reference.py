"""``pr_adam_step`` (csrc/optim.hip) restated in numpy, twice, with an error bound derived from the formula.

``adam_step_float64`` is one Adam / AdamW update in float64, in the order written at the top of csrc/optim.hip: unscale, maximize, L2
or decoupled decay, ``m``, ``v``, bias corrections, ``p``.  The hyper-parameters enter as the float32 values the C ABI receives
(``f32(0.9)``), so the reference and the kernel solve the same problem.  ``adam_step_fp32`` is the same update in ``np.float32``, one
rounding per operation, in the kernel's order and association: what honest fp32 arithmetic gives (the library is built with
``-ffp-contract=off``).  No torch, no GPU.

The tolerances (returned by ``adam_step_float64``) bound |fp32 result - float64 result| element by element.  Notation: ``u = 2^-24`` (the
relative error of one fp32 rounding), ``tiny = 2^-126`` (covers roundings into the subnormal range), ``g`` the gradient after unscaling,
sign and L2 decay, ``g_abs = |grad / scale| + weight_decay |p_old|`` (L2 mode; the scale of the operands, not of a sum that may cancel),
``gm = g_abs + |m_old|``.

* ``g`` carries at most 3 roundings relative to ``g_abs`` (``1 / scale``, the product with it, the L2 sum; the L2 product is inside).
* ``m = m + (1 - beta1) (g - m)``: ``1 - beta1`` is exact (Sterbenz for beta1 >= 0.5, trivially for 0).  The difference, the product and
  the sum round once each on quantities no larger than ``gm``, plus the error of ``g``:  ``tol_m = 4u gm + tiny``.
* ``v = beta2 v + ((1 - beta2) g) g``: two products and a sum on ``(1 - beta2) g^2``, one product and the sum on ``beta2 v``, and
  ``2 x 3u`` relative from ``g`` squared, all weighted by ``1 - beta2`` or ``beta2`` <= 1:  ``tol_v = 6u (v_old + g_abs^2) + tiny``.
* the denominator ``sqrt(v) / bc2_sqrt + eps``: the smallest value fp32 can reach is the square root of the smallest ``v``, with the
  roundings of ``sqrtf``, of ``bc2_sqrt`` (a float conversion and a ``sqrtf``: 1.5u), of the division and of the sum (u each, and u on
  ``eps`` as the sum's other operand):  ``den_lo = sqrt(max(v_ref - tol_v, 0)) / bc2_sqrt (1 - 6u) + eps (1 - 2u)``.
  The error of ``v`` goes through the square root: when ``g + weight_decay p`` cancels, ``tol_v`` may be as large as ``v`` itself, which is
  why the denominator is propagated instead of bounded relative to the result.
* the update ``(step_size m) / den``, ``step_size = lr / bc1`` with ``bc1`` a float conversion (2u), the product and the quotient (2u), and
  two more for the margin:  ``upd_hi = step_size (1 + 2u) (|m_ref| + tol_m) / den_lo (1 + 4u)``,  against  ``upd = step_size |m_ref| / den_ref``.
  (The largest deviation is on the side of the small denominator: ``1 / den`` is convex.)
* ``p``: the decoupled decay ``p - (lr weight_decay) p`` rounds three times on at most ``|p_old|``, the final difference once on at most
  ``|p_old| + upd_hi``:  ``tol_p = (upd_hi - upd) + u (4 |p_old| + 2 upd_hi) + tiny``.

tests/test_adam_cpu.py holds ``adam_step_fp32`` to these tolerances on the GPU tests' own inputs (gradients and moments from 1e-12 to 1e6,
zero state, ``m`` close to ``g``, every mode below, t from 1 to 2^24, scales 65536 / 3 / 1e-3); its worst error there is 0.47, 0.54 and 0.61
of ``tol_p``, ``tol_m`` and ``tol_v``."""
from typing import NamedTuple, Optional

import numpy as np

F = np.float32
U = 2.0 ** -24
TINY = 2.0 ** -126


def f32(x) -> float:
    """The float32 value the C ABI receives for a hyper-parameter, as a Python float."""
    return float(np.float32(x))


class AdamStep(NamedTuple):
    p: np.ndarray
    m: np.ndarray
    v: np.ndarray
    step_device: Optional[np.float32]      # the device count after the call (None: the count came by value)
    tol_p: Optional[np.ndarray] = None
    tol_m: Optional[np.ndarray] = None
    tol_v: Optional[np.ndarray] = None


def _skipped(found_inf) -> bool:
    return found_inf is not None and not (float(found_inf) == 0.0)          # (a NaN is "not zero": skipped, like the kernel's != 0.f)


def adam_step_float64(p, g, m, v, *, lr, beta1, beta2, eps, weight_decay=0.0, decoupled=False, maximize=False, step=None,
                      step_device=None, grad_scale=None, found_inf=None) -> AdamStep:
    """One update in float64 from fp32 (or float64) inputs.  ``step``: the count AFTER this update, by value; or ``step_device``: the fp32
    count BEFORE it, incremented in fp32 first (returned as ``step_device``).  ``grad_scale``: the gradients are divided by it;
    ``found_inf``: a non-zero value (a NaN included) leaves everything as it is, the device count included."""
    assert (step is None) != (step_device is None)
    p0, g0, m0, v0 = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    zero = np.zeros_like(p0)
    if _skipped(found_inf):
        return AdamStep(p0.copy(), m0.copy(), v0.copy(), None if step_device is None else F(step_device), zero, zero.copy(), zero.copy())
    lr, beta1, beta2, eps, weight_decay = f32(lr), f32(beta1), f32(beta2), f32(eps), f32(weight_decay)
    new_count = None if step_device is None else F(F(step_device) + F(1.0))
    t = float(step) if step_device is None else float(new_count)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        g = g0 if grad_scale is None else g0 / float(F(grad_scale))
        g_abs = np.abs(g)
        if maximize:
            g = -g
        p1 = p0
        if weight_decay != 0.0:
            if decoupled:
                p1 = p0 - lr * weight_decay * p0
            else:
                g = g + weight_decay * p0
                g_abs = g_abs + weight_decay * np.abs(p0)
        m1 = m0 + (1.0 - beta1) * (g - m0)
        v1 = beta2 * v0 + (1.0 - beta2) * g * g
        bc1 = 1.0 - beta1 ** t
        bc2_sqrt = np.sqrt(1.0 - beta2 ** t)
        step_size = lr / bc1
        den = np.sqrt(v1) / bc2_sqrt + eps
        p2 = p1 - step_size * m1 / den
        # the tolerances (module docstring)
        gm = g_abs + np.abs(m0)
        tol_m = 4 * U * gm + TINY
        tol_v = 6 * U * (v0 + g_abs * g_abs) + TINY
        den_lo = np.sqrt(np.maximum(v1 - tol_v, 0.0)) / bc2_sqrt * (1 - 6 * U) + eps * (1 - 2 * U)
        upd = step_size * np.abs(m1) / den
        upd_hi = step_size * (1 + 2 * U) * (np.abs(m1) + tol_m) / den_lo * (1 + 4 * U)
        tol_p = (upd_hi - upd) + U * (4 * np.abs(p0) + 2 * upd_hi) + TINY
    return AdamStep(p2, m1, v1, new_count, tol_p, tol_m, tol_v)


def adam_step_fp32(p, g, m, v, *, lr, beta1, beta2, eps, weight_decay=0.0, decoupled=False, maximize=False, step=None,
                   step_device=None, grad_scale=None, found_inf=None, corrections=None) -> AdamStep:
    """The same update in ``np.float32``: one rounding per operation, the kernel's order and association.  ``1 / scale`` is read once
    and multiplied by; the corrections are ``float32(1 - beta1**t)`` and ``sqrt(float32(1 - beta2**t))`` with the powers in double
    (``corrections``: a function ``(beta1, beta2, t) -> (bc1, bc2_sqrt)`` that replaces them - how a test shows what a float ``powf`` costs)."""
    assert (step is None) != (step_device is None)
    p, g, m, v = (np.array(a, dtype=F) for a in (p, g, m, v))
    if _skipped(found_inf):
        return AdamStep(p, m, v, None if step_device is None else F(step_device))
    lr, beta1, beta2, eps, weight_decay = F(lr), F(beta1), F(beta2), F(eps), F(weight_decay)
    one = F(1.0)
    new_count = None if step_device is None else F(F(step_device) + one)
    t = float(step) if step_device is None else float(new_count)
    bc1 = F(1.0 - float(beta1) ** t)
    bc2_sqrt = np.sqrt(F(1.0 - float(beta2) ** t))
    if corrections is not None:
        bc1, bc2_sqrt = (F(c) for c in corrections(beta1, beta2, t))
    step_size = F(lr / bc1)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore", under="ignore"):
        if grad_scale is not None:
            g = g * F(one / F(grad_scale))
        if maximize:
            g = -g
        if weight_decay != 0:
            if decoupled:
                p = p - F(lr * weight_decay) * p
            else:
                g = g + weight_decay * p
        m = m + F(one - beta1) * (g - m)
        v = beta2 * v + (F(one - beta2) * g) * g
        den = np.sqrt(v) / bc2_sqrt + eps
        p = p - (step_size * m) / den
    assert p.dtype == m.dtype == v.dtype == F and type(step_size) is F and type(bc2_sqrt) is F
    return AdamStep(p, m, v, new_count)


# ---------------------------------------------------------------------------------------------------------------------
# the inputs of the tests (CPU and GPU draw the same ones)
FAMILIES = ("wide", "zero_state", "m_near_g")


def inputs(family: str, n: int, seed: int):
    """``p, g, m, v`` as fp32 arrays of ``n`` elements.  ``wide``: gradients and moments of both signs from 1e-12 to 1e6, second moments from
    1e-12 to 1e6, a few exact zeros; ``zero_state``: the first step of a training run; ``m_near_g``: ``m`` within a few ulp of ``g`` (the
    difference ``g - m`` cancels) and ``v`` close to ``g^2``.  Parameters: normal draws scaled by 1e-3 to 10."""
    rng = np.random.default_rng([seed, FAMILIES.index(family), n])
    signed = lambda: rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-12, 6, n)
    p = (rng.normal(size=n) * 10.0 ** rng.uniform(-3, 1, n)).astype(F)
    g = signed().astype(F)
    if family == "wide":
        m, v = signed().astype(F), (10.0 ** rng.uniform(-12, 6, n)).astype(F)
        zeros = rng.random(n) < 0.02
        g[zeros & (rng.random(n) < 0.5)] = 0
        m[zeros] = 0
        v[zeros & (rng.random(n) < 0.5)] = 0
    elif family == "zero_state":
        m, v = np.zeros(n, F), np.zeros(n, F)
    elif family == "m_near_g":
        m = (g.astype(np.float64) * (1 + rng.integers(-3, 4, n) * 2.0 ** -23)).astype(F)
        v = (g.astype(np.float64) ** 2 * (1 + rng.normal(size=n) * 1e-3)).astype(F)
    else:
        raise ValueError(family)
    return p, g, m, v


BASE = dict(lr=3e-3, beta1=0.9, beta2=0.999, eps=1e-8)
MODES = {
    "plain": dict(BASE),
    "l2": dict(BASE, weight_decay=0.05),
    "decoupled": dict(BASE, weight_decay=0.05, decoupled=True),
    "maximize": dict(BASE, maximize=True),
    "maximize_l2": dict(BASE, weight_decay=0.05, maximize=True),
    "beta1_zero": dict(BASE, beta1=0.0),
    "beta2_zero": dict(BASE, beta2=0.0),
    "betas_zero_decoupled": dict(BASE, beta1=0.0, beta2=0.0, weight_decay=0.1, decoupled=True),
    "eps_tiny": dict(BASE, eps=1e-15),
    "eps_large_l2": dict(BASE, eps=1e-3, weight_decay=0.5),
    "lr_one": dict(BASE, lr=1.0),           # the update dominates the parameter: the corrections' last digits show
    "beta2_near_one": dict(BASE, lr=1.0, beta2=0.99999),      # 1 - beta2^t cancels five digits at small t: the power has to be a double's
}
STEPS = (1, 2, 3, 1000, 100000, 2 ** 24)
SCALES = (65536.0, 3.0, 1e-3)
SIZES = (1, 3, 4, 5, 255, 1023, 1024, 1025, 4099)


def ratios(got: AdamStep, want: AdamStep):
    """``max |got - want| / tolerance`` for ``p, m, v`` over the elements whose reference is finite."""
    out = []
    for key in ("p", "m", "v"):
        ref, tol = getattr(want, key), getattr(want, "tol_" + key)
        finite = np.isfinite(ref) & np.isfinite(tol)
        err = np.abs(np.asarray(getattr(got, key), np.float64)[finite] - ref[finite])
        with np.errstate(invalid="ignore", divide="ignore"):
            r = np.where(err == 0, 0.0, err / tol[finite])        # (a skipped update: tolerance 0, error 0)
        out.append(float(np.nan_to_num(r, nan=np.inf).max()) if r.size else 0.0)
    return tuple(out)
