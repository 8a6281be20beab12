"""Per-entry acceptance of an optimizer step (the convention of tests/grad_checks.py applied to AdamW / Lion).

witness   = the same rule in fp64 (torch.optim.AdamW on float64 CPU tensors / the Lion rule in numpy float64)
reference = the rule in fp32 on the CPU (torch.optim.AdamW float32 / the Lion rule in numpy float32)
scale_i   = sum of the absolute values of the entry's own terms, from the witness
r_ref     = max_i |ref_i - wit_i| / scale_i, floored at 2^-24
accepted  iff |k_i - wit_i| <= 4 r_ref scale_i for EVERY entry (4 x the reference's own fp32 error: DESIGN §7).

An ulp-of-the-value criterion is useless here: cancellation in exp_avg gives the fp32 reference itself ~1e6 ulp on single
entries, which is why the bound is on the terms."""

from __future__ import annotations

import numpy as np
import torch

FLOOR = 2.0 ** -24
MARGIN = 4.0


def adamw_trajectory(p0, grads, coefs, lr, wd, betas=(0.9, 0.999), eps=1e-8, dtype=torch.float64, m0=None, v0=None, step0=0):
    """torch.optim.AdamW (foreach=False) on CPU tensors of `dtype`; gradients are multiplied by `coefs[k]` in that dtype first.
    Returns per step (p, exp_avg, exp_avg_sq) as numpy arrays, and per step the term scales computed in float64 from the state
    BEFORE the step (meaningful for the float64 run)."""
    p = torch.nn.Parameter(torch.from_numpy(np.asarray(p0)).to(dtype).clone())
    opt = torch.optim.AdamW([p], lr=lr, betas=betas, eps=eps, weight_decay=wd, foreach=False)
    if m0 is not None:
        opt.state[p] = {"step": torch.tensor(float(step0)), "exp_avg": torch.from_numpy(np.asarray(m0)).to(dtype).clone(),
                        "exp_avg_sq": torch.from_numpy(np.asarray(v0)).to(dtype).clone()}
    out, scales = [], []
    b1, b2 = betas
    for k, (g, c) in enumerate(zip(grads, coefs)):
        step = step0 + k + 1
        g_t = torch.from_numpy(np.asarray(g)).to(dtype) * torch.tensor(c, dtype=torch.float32).to(dtype)
        st = opt.state.get(p, {})
        p_old = p.detach().double().numpy().copy()
        m_old = st["exp_avg"].double().numpy().copy() if "exp_avg" in st else np.zeros_like(p_old)
        v_old = st["exp_avg_sq"].double().numpy().copy() if "exp_avg_sq" in st else np.zeros_like(p_old)
        p.grad = g_t.clone()
        opt.step()
        st = opt.state[p]
        out.append((p.detach().numpy().copy(), st["exp_avg"].numpy().copy(), st["exp_avg_sq"].numpy().copy()))
        g64 = g_t.double().numpy()
        m_new = b1 * m_old + (1 - b1) * g64
        v_new = b2 * v_old + (1 - b2) * g64 * g64
        denom = np.sqrt(v_new) / np.sqrt(1 - b2 ** step) + eps
        step_size = lr / (1 - b1 ** step)
        scales.append((np.abs(p_old) + np.abs(lr * wd * p_old) + np.abs(step_size * m_new / denom),
                       np.abs(b1 * m_old) + np.abs((1 - b1) * g64),
                       np.abs(b2 * v_old) + np.abs((1 - b2) * g64 * g64)))
    return out, scales


def lion_trajectory(p0, m0, grads, coefs, lr, wd, betas=(0.9, 0.99), dtype=np.float64):
    """The reference's Lion rule (decay, sign(b1 m + (1-b1) g), b2 average) in numpy `dtype`, written with separate operations."""
    f = dtype
    p, m = np.asarray(p0).astype(f), np.asarray(m0).astype(f)
    b1, b2 = betas
    out, scales = [], []
    for g, c in zip(grads, coefs):
        g = np.asarray(g).astype(f) * f(np.float32(c))
        p_old, m_old = p.astype(np.float64), m.astype(np.float64)
        p = p * f(1 - lr * wd)
        update = m * f(b1) + g * f(1 - b1)
        terms = np.abs(m * f(b1)) + np.abs(g * f(1 - b1))
        decided = np.abs(update) > 1e-6 * terms  # the sign is not within rounding of zero
        p = p + np.sign(update) * f(-lr)
        m = m * f(b2) + g * f(1 - b2)
        out.append((p.copy(), m.copy(), decided))
        g64 = g.astype(np.float64)
        scales.append((np.abs(p_old) + np.abs(lr * wd * p_old) + lr, np.abs(b2 * m_old) + np.abs((1 - b2) * g64)))
    return out, scales


def check_entries(name: str, kernel, reference, witness, scale, r_ref: float | None = None, keep=None) -> float:
    """Assert the per-entry bound; returns r_ref.  Prints the observed maximum of |k - wit| / (r_ref scale) (<= 4 passes).
    `r_ref`: use this value (an edge subset is held to the r_ref of the whole tensor set).  `keep`: boolean mask of the entries
    that take part (Lion: entries whose sign is decided)."""
    k, ref, wit, scale = (np.asarray(a, dtype=np.float64).ravel() for a in (kernel, reference, witness, scale))
    assert k.shape == ref.shape == wit.shape == scale.shape, (name, k.shape, ref.shape, wit.shape, scale.shape)
    assert np.all(np.isfinite(k)), f"{name}: non-finite entries in the result"
    if keep is not None:
        keep = np.asarray(keep, dtype=bool).ravel()
        k, ref, wit, scale = k[keep], ref[keep], wit[keep], scale[keep]
    live = scale > 0
    if r_ref is None:
        r_ref = max(float(np.max(np.abs(ref - wit)[live] / scale[live], initial=0.0)), FLOOR)
    err = np.abs(k - wit)
    assert np.all(err[~live] == 0), f"{name}: an entry whose terms are all zero moved"
    ratio = float(np.max(err[live] / (r_ref * scale[live]), initial=0.0))
    worst = int(np.argmax(np.where(live, err / np.where(live, r_ref * scale, 1.0), 0.0)))
    print(f"[optim] {name}: r_ref = {r_ref:.3e}, max |k - wit| / (r_ref scale) = {ratio:.3f} at entry {worst} of {k.size}")
    assert ratio <= MARGIN, f"{name}: entry {worst}: |k - wit| = {err[worst]:.3e} > 4 x {r_ref:.3e} x {scale[worst]:.3e}"
    return r_ref


def log_uniform_grads(rng, n: int, steps: int, sign=None):
    """N(0, 1) x a log-uniform scale 1e-6 ... 1 per entry and step."""
    out = []
    for _ in range(steps):
        g = rng.normal(0.0, 1.0, n) * 10.0 ** rng.uniform(-6.0, 0.0, n)
        out.append((np.abs(g) * sign if sign is not None else g).astype(np.float32))
    return out
