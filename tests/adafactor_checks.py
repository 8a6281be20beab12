"""Per-entry acceptance of an Adafactor step (the convention of tests/optim_checks.py).

witness   = transformers.Adafactor(relative_step=False, scale_parameter=False) on float64 CPU tensors, the gradient multiplied
            by float32(coef) first; its parameter and state are kept per step
reference = the SAME library class on float32 CPU tensors, every step started from the witness's state before that step
scale_i   = sum of the absolute values of the entry's own terms, from the witness's state before the step:
              parameter       |p| + |wd lr p| + |lr u / denom|
              row / col / v   |beta2t old| + |(1 - beta2t) mean(sq)|        (v: sq itself)
r_ref     = max_i |ref_i - wit_i| / scale_i, floored at 2^-24
accepted  iff |k_i - wit_i| <= 4 r_ref scale_i for EVERY entry.

Why the reference restarts from the witness every step.  Run as one fp32 trajectory, the library shows up to 6e-5 of
|p_old| + |delta| on single entries of steps 2 and 3 (shapes (67, 129) and (1000,), log-uniform gradients) while step 1 and all
state tensors agree with fp64 to ~2e-7.  No operation is at fault: rsqrt, the moving average, norm and the square each agree
with fp64 to <= 2e-7 on their own.  The entries are those whose parameter passed close to zero on an EARLIER step (|p_old| one to
three decades below |p_0|): the rounding error of that earlier step, 1e-7 of the terms it had then, is carried in p_old and is
measured against the far smaller terms of the current step.  It is a property of comparing trajectories with a per-step scale,
not of the fp32 rule, and the kernel's own trajectory has it as well.  Started from the witness's state, the library's fp32 step
stays within 5.3e-7 of the scale on every entry of every step (factored; 1.9e-7 unfactored).  So the library itself is the honest
fp32 statement, step by step, and the code under test is checked the same way: each of its steps starts from the witness's
state (rounded to fp32) and is compared with the witness after that step.  The bound is not widened.

`restated_step` is the rule in numpy with separate operations.  It is NOT the reference: it exists so that the host test can
seed mistakes and see the checker flag them (and, unseeded in float64, must reproduce the witness to 1e-12)."""

from __future__ import annotations

import math

import numpy as np
import torch

from optim_checks import FLOOR, MARGIN, check_entries, log_uniform_grads  # noqa: F401  (re-exported for the tests)

HYPER = dict(eps1=1e-30, clip_threshold=1.0, decay_rate=-0.8)
STATE_KEYS = ("exp_avg_sq_row", "exp_avg_sq_col", "exp_avg_sq")


def _library(p, state, step_before, dtype, lr, wd, hyper):
    from transformers.optimization import Adafactor

    param = torch.nn.Parameter(torch.from_numpy(np.asarray(p)).to(dtype).clone())
    opt = Adafactor([param], lr=lr, eps=(hyper["eps1"], 1e-3), clip_threshold=hyper["clip_threshold"], decay_rate=hyper["decay_rate"], beta1=None,
                    weight_decay=wd, relative_step=False, scale_parameter=False)
    if step_before > 0:
        opt.state[param] = {"step": step_before, "RMS": 0, **{k: torch.from_numpy(np.asarray(v)).to(dtype).clone() for k, v in state.items()}}
    return param, opt


def _snapshot(param, opt):
    st = opt.state[param]
    return {"p": param.detach().numpy().copy(), **{k: st[k].numpy().copy() for k in STATE_KEYS if k in st}}


def library_step(before: dict, g, coef, step: int, lr, wd, dtype=torch.float32, hyper=HYPER) -> dict:
    """One step of transformers' Adafactor in `dtype` from the state `before` ({"p", state keys}; step 1: only "p")."""
    param, opt = _library(before["p"], {k: v for k, v in before.items() if k != "p"}, step - 1, dtype, lr, wd, hyper)
    param.grad = torch.from_numpy(np.asarray(g)).to(dtype) * torch.tensor(coef, dtype=torch.float32).to(dtype)
    opt.step()
    return _snapshot(param, opt)


def _terms(before: dict, g, coef, step: int, lr, wd, hyper):
    """float64 numpy: the scales of one step and the witness's rms / clip_threshold, from the state before the step."""
    p = np.asarray(before["p"], dtype=np.float64)
    g = np.asarray(g, dtype=np.float64) * float(np.float32(coef))
    b2 = 1.0 - math.pow(step, hyper["decay_rate"])
    sq = g * g + hyper["eps1"]
    scales = {}
    if p.ndim >= 2:
        row0 = np.asarray(before.get("exp_avg_sq_row", np.zeros(p.shape[:-1])), dtype=np.float64)
        col0 = np.asarray(before.get("exp_avg_sq_col", np.zeros(p.shape[:-2] + p.shape[-1:])), dtype=np.float64)
        scales["exp_avg_sq_row"] = np.abs(b2 * row0) + np.abs((1 - b2) * sq.mean(-1))
        scales["exp_avg_sq_col"] = np.abs(b2 * col0) + np.abs((1 - b2) * sq.mean(-2))
        row, col = b2 * row0 + (1 - b2) * sq.mean(-1), b2 * col0 + (1 - b2) * sq.mean(-2)
        u = (1.0 / np.sqrt(row / row.mean(-1, keepdims=True)))[..., None] * (1.0 / np.sqrt(col))[..., None, :] * g
    else:
        v0 = np.asarray(before.get("exp_avg_sq", np.zeros(p.shape)), dtype=np.float64)
        scales["exp_avg_sq"] = np.abs(b2 * v0) + np.abs((1 - b2) * sq)
        u = g / np.sqrt(b2 * v0 + (1 - b2) * sq)
    ratio = math.sqrt(float(np.mean(u * u))) / hyper["clip_threshold"] if u.size else 0.0
    scales["p"] = np.abs(p) + np.abs(wd * lr * p) + np.abs(lr * u / max(1.0, ratio))
    return scales, ratio


def adafactor_record(before: dict, g, coef, step: int, lr, wd, hyper=HYPER) -> dict:
    """Everything a check of ONE step from the state `before` needs: {"before", "wit" (after the step, float64), "ref" (the float32
    library step from `before`), "scale", "ratio" (the witness's rms / clip_threshold), "step", "g", "coef"}."""
    before = {k: np.asarray(v, dtype=np.float64) for k, v in before.items()}
    wit = library_step(before, g, coef, step, lr, wd, torch.float64, hyper)
    ref = library_step(before, g, coef, step, lr, wd, torch.float32, hyper)
    scales, ratio = _terms(before, g, coef, step, lr, wd, hyper)
    return {"before": before, "wit": wit, "ref": ref, "scale": scales, "ratio": ratio, "step": step, "g": np.asarray(g), "coef": coef}


def adafactor_steps(p0, grads, coefs, lr, wd, hyper=HYPER, p_round=None):
    """The witness trajectory as one record per step.  `p_round`: what the parameter is rounded to between steps (a bf16 parameter
    without master weights: the rule itself stores the rounded value)."""
    out = []
    before = {"p": np.asarray(p0, dtype=np.float64)}
    for k, (g, c) in enumerate(zip(grads, coefs)):
        out.append(adafactor_record(before, g, c, k + 1, lr, wd, hyper))
        before = dict(out[-1]["wit"])
        if p_round is not None:
            before["p"] = p_round(before["p"])
    return out


def check_step(name: str, got: dict, rec: dict, r_ref: dict | None = None, extra_abs=None) -> dict:
    """Every entry of the parameter and of each state tensor of one step under the bound; returns {key: r_ref}.
    `extra_abs`: an absolute allowance per parameter entry on top of the bound (half a bf16 ulp of the result without master weights)."""
    out = {}
    for key in rec["wit"]:
        wit, scale = rec["wit"][key], rec["scale"][key]
        k = np.asarray(got[key], dtype=np.float64)
        if extra_abs is not None and key == "p":  # the allowance is taken off the error before the bound is applied
            err = np.maximum(np.abs(k.ravel() - wit.ravel()) - np.asarray(extra_abs, dtype=np.float64).ravel(), 0.0)
            k = (wit.ravel() + err).reshape(wit.shape)
        out[key] = check_entries(f"{name} {key}", k, rec["ref"][key], wit, scale, r_ref=None if r_ref is None else r_ref[key])
    return out


def restated_step(before: dict, g, coef, step: int, lr, wd, dtype=np.float32, hyper=HYPER, mistake: str | None = None) -> dict:
    """The rule in numpy `dtype` with separate operations; `mistake` seeds one defect (tests of the checker)."""
    f = dtype
    with np.errstate(divide="ignore", invalid="ignore"):  # (a seeded mistake may divide by zero: the checker sees the non-finite result)
        return _restated_step(before, g, coef, step, lr, wd, f, hyper, mistake)


def _restated_step(before, g, coef, step, lr, wd, f, hyper, mistake):
    p = np.asarray(before["p"]).astype(f)
    raw = np.asarray(g).astype(f)
    c = f(np.float32(coef))
    g = raw * c
    b2 = 1.0 - math.pow(step - 1 if mistake == "beta2t_from_previous_step" else step, hyper["decay_rate"])
    eps1 = f(0.0) if mistake == "eps1_dropped" else f(hyper["eps1"])
    sq = (raw * raw) * c + eps1 if mistake == "coef_after_square" else g * g + eps1
    out = {}
    if p.ndim >= 2:
        row = np.asarray(before.get("exp_avg_sq_row", np.zeros(p.shape[:-1]))).astype(f)
        col = np.asarray(before.get("exp_avg_sq_col", np.zeros(p.shape[:-2] + p.shape[-1:]))).astype(f)
        over_cols, over_rows = (sq.mean(-2), sq.mean(-1)) if mistake == "mean_over_wrong_axis" else (sq.mean(-1), sq.mean(-2))
        row = row * f(b2) + over_cols.astype(f) * f(1 - b2)
        col = col * f(b2) + over_rows.astype(f) * f(1 - b2)
        rf = f(1) / np.sqrt(row if mistake == "row_factor_not_normalised" else row / row.mean(-1, keepdims=True).astype(f))
        u = (rf[..., None] * (f(1) / np.sqrt(col))[..., None, :]) * g
        out["exp_avg_sq_row"], out["exp_avg_sq_col"] = row, col
    else:
        v = np.asarray(before.get("exp_avg_sq", np.zeros(p.shape))).astype(f)
        v = v * f(b2) + sq * f(1 - b2)
        u = (f(1) / np.sqrt(v)) * g
        out["exp_avg_sq"] = v
    if mistake == "rms_per_matrix" and p.ndim > 2:
        rms = np.sqrt((u.astype(np.float64) ** 2).mean(axis=(-1, -2), keepdims=True)).astype(f)
    else:
        rms = f(math.sqrt(float((u.astype(np.float64) ** 2).mean())))
    denom = f(1) if mistake == "update_clip_omitted" else np.maximum(f(1), rms / f(hyper["clip_threshold"]))
    u = (u / denom) * f(lr)
    if mistake == "decay_after_update":
        p = p - u
        p = p + p * f(-wd * lr)
    else:
        if wd != 0:
            p = p + p * f(-wd * lr)
        p = p - u
    out["p"] = p.astype(f)
    return out


def clip_case_grads(kind: str, rng, shape, steps: int = 3):
    """Gradients that put the witness's rms(update) / clip_threshold on one side of 1 from step 2 on: one log-uniform magnitude per
    entry, fresh signs per step, every step 10 x smaller ("below": the averages remember larger squares, |u| < 1) or 10 x larger
    ("above": u -> 1 / sqrt(1 - beta2t) > 1).  Step 1 has rms = 1 up to eps1 by construction whatever the gradients are."""
    n = int(np.prod(shape))
    base = np.abs(log_uniform_grads(rng, n, 1)[0]).astype(np.float64)
    factor = {"below": 0.1, "above": 10.0}[kind]
    return [(base * factor ** k * np.where(rng.random(n) < 0.5, -1.0, 1.0)).astype(np.float32).reshape(shape) for k in range(steps)]
