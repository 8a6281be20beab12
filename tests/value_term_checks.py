"""Per-entry check of the value-head (actor-critic) branch (plain numpy; no kernel runs here, nothing of the package is imported).

Why: with a value head the `advantages` column of the policy term, d value_loss / d value and five statistics come out of
`value_head_partial_kernel` / `value_head_finalize_kernel` (csrc/prl_value.hip).  The suite held the statistics to
`1e-4 max(1, |want|)` and the gradient to `rtol=1e-5` of the fp32 oracle on one packed row; here every entry and every statistic is
measured against the size of its own terms, on packed rows and on [B, L] batches.

The witness (`witness`) restates reference rl/__init__.py:265-272, 367-381, 441-448 for an unshifted batch.  Entry i = (row, c) of
`value` is paired with target t = i + 1 of the same row; column cols - 1 has no target, column 0 of the targets no prediction.  The
inputs are the fp32 arrays as the device sees them (a bf16 prediction is rounded before it gets here).  In fp32, as the kernel forms
them (build.py compiles with `-ffp-contract=off` and nothing that relaxes division, so these are the IEEE results numpy forms):

    adv[row, 0] = 0      adv[t] = fp32(r_t - v_i)                          every position, labelled or not (:272)
    w_t = 1 / group_tokens_t  or  token_weight = 1 / batch_size;  then w_t * (1 - overflow_t) with overlong_filtering

and in fp64 of those fp32 values, on the labelled targets (labels_t != -100):

    el   = (0.5 (v - r)^2) w              want_i = (v - r) w  where el is a finite fp32 number, 0 elsewhere
    loss = sum nan_to_num(el)             mean = sum nan_to_num(v / num_labels)     mse = sum nan_to_num((v - r)^2 / num_labels)
    max / min = the largest / smallest labelled v, NaN as soon as one of them is NaN (torch's tensor.max());  all five 0.0 without a label

`el is a finite fp32 number` is decided from the fp64 values against FLT_MAX at every step the fp32 evaluation takes (v - r, its
square, the half, the product with w): an intermediate above FLT_MAX is inf from there on, as it is in fp32.  nan_to_num maps NaN -> 0
and +-inf -> +-FLT_MAX, like sum_sum (rl/utils.py:26-31).  No token is left out of a comparison; instead the witness REFUSES a case
(`BadCase`) in which one of those intermediates of a labelled token lies within GUARD (relative) of FLT_MAX - there the decision would
hang on fp32 rounding and the case is badly built.

Metrics.  `check_advantages`: bit for bit, NaN where the witness is NaN.  `check_grad`: |got - want| / ((|v| + |r|) |w|), the size of the
terms of `v - r` before they cancel; exactly 0 where that scale is 0 or not a number: unlabelled targets, the last column, w == 0,
non-finite tokens.  `check_stats`: value_mean against sum |v / num_labels|, value_mse and value_loss against the sum itself (their terms
are non-negative), value_max / value_min exactly; `value_loss_out` is the fp32 cast of the fp64 statistic.

Bounds.  None comes from a kernel.  VALUE_GRAD_BOUND / VALUE_STAT_BOUND / VALUE_LOSS_BOUND = 4 x the largest value of the same metric
for the oracle's own fp32 path (`oracle.rl_loss.token_loss(value=...)`: the reference restated in fp32, pinned to it by goldens c18-c23,
summing per segment in fp32 like sum_sum) over every case of tests/test_gpu_value_edges.py, measured on the CPU (VALUE_REF, rounded up to
two digits; tests/test_value_term_checks_host.py re-measures it and fails if the oracle exceeds what is written).  4 x is the project's
standing margin.  A gradient x 1.0003 scores 3e-4 on a token whose terms do not cancel: no bound may reach that (asserted).
"""

from __future__ import annotations

import dataclasses

import numpy as np

F32 = np.float32
FLT_MAX = float(np.finfo(np.float32).max)
GUARD = 1e-6
MUTANT_FLOOR = 3e-4  # what "gradient x 1.0003" scores
VALUE_STAT_KEYS = ("value_mean", "value_max", "value_min", "value_loss", "value_mse")  # reference rl/__init__.py:441-448, in this order

# case of tests/test_gpu_value_edges.py -> (gradient, statistic, loss): the metrics of this module for the oracle's fp32 path against
# the witness, largest value over the case's shapes and weight configurations, measured on the CPU, rounded up to two digits
VALUE_REF = {
    "shapes": (1.2e-7, 1.2e-7, 1.3e-7),     # the ten (rows, cols) x fp32 / bf16 x group normalization x overlong filtering, packed and [B, L]
    "placement": (5.9e-8, 4.5e-8, 1.2e-7),  # labels at column 1, cols - 1, both sides of every row start and segment boundary, column 0 labelled
    "nonfinite": (8.8e-8, 1.1e-7, 1.1e-7),  # NaN, +-inf, 3e19 on a labelled / an unlabelled token, group_tokens == 0 (the ordinary tokens)
    "e2e": (1.2e-7, 8.6e-8, 3.3e-8),        # the predictions of a critic on 1024 packed tokens and on a [3, 341] batch
}
VALUE_GRAD_BOUND = 4.0 * max(v[0] for v in VALUE_REF.values())
VALUE_STAT_BOUND = 4.0 * max(v[1] for v in VALUE_REF.values())
VALUE_LOSS_BOUND = 4.0 * max(v[2] for v in VALUE_REF.values())
assert max(VALUE_GRAD_BOUND, VALUE_STAT_BOUND, VALUE_LOSS_BOUND) < MUTANT_FLOOR


class BadCase(ValueError):
    """A case on which the witness's finite / non-finite decision would hang on fp32 rounding."""


@dataclasses.dataclass
class ValueWitness:
    shape: tuple
    paired: np.ndarray      # [N] bool: entry i has a target (column < cols - 1)
    mask: np.ndarray        # [N] bool: paired and the target is labelled
    finite: np.ndarray      # [N] bool: the fp32 element 0.5 (v - r)^2 w is finite (meaningful on `mask`)
    w32: np.ndarray         # [N] fp32 weight of the target of entry i
    adv: np.ndarray         # [N] fp32, token-aligned: the advantages column
    grad: np.ndarray        # [N] fp64 d value_loss / d value, 0 off `mask & finite`
    scale: np.ndarray       # [N] fp64 (|v| + |r|) |w| on `mask & finite`, 0 elsewhere
    terms: dict             # "value_mean" / "value_mse" / "value_loss" -> [N] fp64 term of every entry, 0 off `mask`
    stats: dict             # the five statistics
    stat_scale: dict        # name -> sum |term| of the three sums
    loss_out: np.float32    # the fp32 cast of stats["value_loss"]


def _flat(a, dtype=F32):
    return np.ascontiguousarray(np.asarray(a), dtype=dtype).reshape(-1)


def _nan_to_num(x):
    return np.where(np.isnan(x), 0.0, np.clip(x, -FLT_MAX, FLT_MAX))


def _f32v(x):
    """The fp32 value of an fp64 intermediate as far as finiteness goes: above FLT_MAX it is +-inf."""
    return np.where(np.abs(x) > FLT_MAX, np.sign(x) * np.inf, x)


def token_weight(config: dict) -> np.float32:
    bs = config.get("batch_size", 0)
    with np.errstate(all="ignore"):
        return (F32(1) / F32(bs)) if bs else F32(np.inf)


def witness(config: dict, labels, value, rewards, group_tokens, num_labels, overflow, guard: bool = True, mutate: str | None = None) -> ValueWitness:
    """The fp64 witness of the module docstring.  `labels` [B, L]; the other columns the same shape, token-aligned.  `mutate`: a WRONG
    rule, for the host test's mutants - "flat_shift" (entry i paired with i + 1 across the row boundary), "no_overflow" (the overlong factor missing from w), "half" (the 0.5 applied to the gradient), "unlabelled_mse" (unlabelled
    targets entering value_mse), "skip_overflow_mean" (an overflowed sequence left out of value_mean), "neighbour_num_labels" (the first
    target of every run of equal num_labels divided by the run before's, where that is not 0)."""
    lab = np.asarray(labels)
    B, L = lab.shape
    N = B * L
    v, r, gt, nl, ovf = _flat(value), _flat(rewards), _flat(group_tokens), _flat(num_labels), _flat(overflow)
    assert all(a.size == N for a in (v, r, gt, nl, ovf))
    col = np.tile(np.arange(L), B)
    paired = col + 1 < L
    if mutate == "flat_shift":
        paired = np.arange(N) + 1 < N
    tgt = np.minimum(np.arange(N) + 1, N - 1)  # where `paired` is false the target is not used
    labelled = lab.reshape(-1)[tgt] != -100
    mask = paired & labelled
    rt, gtt, nlt, ovt = r[tgt], gt[tgt], nl[tgt], ovf[tgt]
    if mutate == "neighbour_num_labels":
        prev = np.concatenate([nlt[:1], nlt[:-1]])
        nlt = np.where((nlt != prev) & (prev > 0), prev, nlt).astype(F32)
    with np.errstate(all="ignore"):
        adv = np.zeros(N, dtype=F32)
        adv[1:] = (r[1:] - v[:-1]).astype(F32)
        adv[col == 0] = F32(0)
        w32 = (F32(1) / gtt).astype(F32) if config.get("group_normalization", False) else np.full(N, token_weight(config), dtype=F32)
        if config.get("overlong_filtering", False) and mutate != "no_overflow":
            w32 = (w32 * (F32(1) - ovt)).astype(F32)
        v64, r64, w, nl64 = v.astype(np.float64), rt.astype(np.float64), w32.astype(np.float64), nlt.astype(np.float64)
        steps = [_f32v(v64 - r64)]
        steps.append(_f32v(steps[0] * steps[0]))
        steps.append(_f32v(0.5 * steps[1]))
        steps.append(_f32v(steps[2] * w))
        diff, sq, el = steps[0], steps[1], steps[3]
        if guard:
            raw = [v64 - r64, diff * diff, 0.5 * sq, steps[2] * w]
            for name, x in zip(("v - r", "(v - r)^2", "0.5 (v - r)^2", "0.5 (v - r)^2 w"), raw):
                near = mask & (np.abs(np.abs(x) - FLT_MAX) <= GUARD * FLT_MAX)
                if near.any():
                    i = int(np.flatnonzero(near)[0])
                    raise BadCase(f"entry {i}: {name} = {x[i]!r} is within {GUARD:g} of FLT_MAX")
        finite = np.isfinite(el)
        live = mask & finite
        grad = np.where(live, ((0.5 if mutate == "half" else 1.0) * (v64 - r64)) * w, 0.0)
        scale = np.where(live, (np.abs(v64) + np.abs(r64)) * np.abs(w), 0.0)
        scale = np.where(np.isfinite(scale), scale, 0.0)
        grad = np.where(scale > 0, grad, 0.0)
        mean_mask = mask & ~(ovt == 1) if mutate == "skip_overflow_mean" else mask
        mse_mask = paired if mutate == "unlabelled_mse" else mask
        terms = {
            "value_mean": np.where(mean_mask, _nan_to_num(_f32v(v64 / nl64)), 0.0),
            "value_mse": np.where(mse_mask, _nan_to_num(_f32v(sq / nl64)), 0.0),
            "value_loss": np.where(mask, _nan_to_num(el), 0.0),
        }
    stats = {k: float(t.sum()) for k, t in terms.items()}
    sel = v[mask]
    with np.errstate(all="ignore"):
        stats["value_max"] = float(np.max(sel)) if sel.size else 0.0  # numpy's max / min return NaN if any element is NaN, like torch's
        stats["value_min"] = float(np.min(sel)) if sel.size else 0.0
        loss_out = F32(stats["value_loss"])
    stat_scale = {k: float(np.abs(t).sum()) for k, t in terms.items()}
    return ValueWitness((B, L), paired, mask, finite, w32, adv, grad, scale, terms, stats, stat_scale, loss_out)


# ---- metrics ------------------------------------------------------------------------------------------------------------
def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=F32).reshape(-1).view(np.uint32)


def check_advantages(got, w: ValueWitness) -> tuple[int, int | None]:
    """(number of entries of the advantages column that are not bit-equal to the witness's - NaN against NaN counts as equal, whatever
    the payload -, first such index)."""
    g = np.ascontiguousarray(got, dtype=F32).reshape(-1)
    assert g.shape == w.adv.shape
    both_nan = np.isnan(g) & np.isnan(w.adv)
    d = (bits(g) != bits(w.adv)) & ~both_nan
    return int(d.sum()), (int(np.flatnonzero(d)[0]) if d.any() else None)


@dataclasses.dataclass
class GradCheck:
    err: float              # max over entries with scale > 0 of |got - want| / scale
    at: int
    got: float
    want: float
    stray: int              # entries that must be exactly 0 and are not (NaN included)
    stray_at: int | None

    def ok(self, bound: float | None = None) -> bool:
        return self.stray == 0 and self.err <= (VALUE_GRAD_BOUND if bound is None else bound)

    def __str__(self):
        s = f"d value error {self.err:.3e} at entry {self.at} (got {self.got:.9e} want {self.want:.9e})"
        return s + (f"; {self.stray} entries must be exactly 0 and are not, first {self.stray_at}" if self.stray else "")


def check_grad(got, w: ValueWitness) -> GradCheck:
    g = np.asarray(got, dtype=np.float64).reshape(-1)
    assert g.shape == w.grad.shape
    live = w.scale > 0
    with np.errstate(all="ignore"):
        rel = np.where(live, np.abs(g - w.grad) / np.where(live, w.scale, 1.0), 0.0)
    rel = np.where(np.isnan(rel), np.inf, rel)
    bad = ~live & ~(g == 0)  # NaN == 0 is false: a NaN counts
    u = int(rel.argmax()) if rel.size else 0
    return GradCheck(float(rel[u]) if rel.size else 0.0, u, float(g[u]) if rel.size else 0.0, float(w.grad[u]) if rel.size else 0.0,
                     int(bad.sum()), int(np.flatnonzero(bad)[0]) if bad.any() else None)


@dataclasses.dataclass
class StatCheck:
    err: float              # max over value_mean / value_mse of |got - want| / sum |term|
    name: str
    loss_err: float         # value_loss: |got - want| / sum of its terms
    mismatch: list          # value_max / value_min that differ, sums that must be exactly 0 and are not, a wrong value_loss_out

    def ok(self, stat_bound: float | None = None, loss_bound: float | None = None) -> bool:
        return (not self.mismatch and self.err <= (VALUE_STAT_BOUND if stat_bound is None else stat_bound)
                and self.loss_err <= (VALUE_LOSS_BOUND if loss_bound is None else loss_bound))

    def __str__(self):
        s = f"statistics {self.err:.3e} ({self.name}); value_loss {self.loss_err:.3e}"
        return s + (f"; differ where they must be equal: {self.mismatch}" if self.mismatch else "")


def _same(a: float, b: float) -> bool:
    return a == b or (np.isnan(a) and np.isnan(b))


def _sum_err(g: float, want: float, sc: float):
    if sc == 0:
        return None if g == 0 else np.inf
    e = abs(g - want) / sc
    return np.inf if np.isnan(e) else e


def check_stats(got: dict, w: ValueWitness, loss_out=None) -> StatCheck:
    """`got`: name -> value for VALUE_STAT_KEYS (a name it does not hold is not checked).  `loss_out`: the fp32 `value_loss_out` of the
    same launch; it must be the fp32 cast of got["value_loss"] (of the witness's where `got` has none)."""
    worst, name, mismatch = 0.0, "-", []
    for k in ("value_mean", "value_mse"):
        if k not in got:
            continue
        e = _sum_err(float(got[k]), w.stats[k], w.stat_scale[k])
        if e is None:
            continue
        if e == np.inf and w.stat_scale[k] == 0:
            mismatch.append(k)
        elif e > worst:
            worst, name = e, k
    for k in ("value_max", "value_min"):
        if k in got and not _same(float(got[k]), w.stats[k]):
            mismatch.append(k)
    loss_err = 0.0
    if "value_loss" in got:
        e = _sum_err(float(got["value_loss"]), w.stats["value_loss"], w.stat_scale["value_loss"])
        if e is not None and w.stat_scale["value_loss"] == 0:
            mismatch.append("value_loss")
        elif e is not None:
            loss_err = e
    if loss_out is not None:
        with np.errstate(all="ignore"):
            cast = F32(got["value_loss"]) if "value_loss" in got else w.loss_out
        if not _same(float(loss_out), float(cast)):
            mismatch.append("value_loss_out")
    return StatCheck(float(worst), name, float(loss_err), mismatch)


# ---- the oracle's own fp32 path on the same arrays (the yardstick of every bound) ---------------------------------------
def oracle_fp32(config: dict, batch: dict, value):
    """`oracle.rl_loss.token_loss(value=...)` on an unshifted batch -> (advantages [N] fp32 token-aligned, d value_loss / d value [N]
    fp32, the five statistics).  The oracle's `g_value` is d loss / d value = value_loss_coef x d value_loss / d value: it is asked with
    a coefficient of 1, which multiplies exactly.  Its advantages live on the shifted axis; column 0 is the 0 the kernel writes.  For a
    batch without a label the oracle returns the reference's one-key dict; the five statistics are then the 0.0 of `.any() else 0.0`."""
    from oracle import rl_loss as orl

    b = dict(batch)
    B, L = b["labels"].shape
    packed = B == 1 and b.get("position_ids") is not None
    b.setdefault("input_ids", np.zeros_like(b["labels"]))
    for k in ("old_logprobs", "ref_logprobs", "advantages"):
        b.setdefault(k, np.zeros((B, L), dtype=F32))
    cfg = dict(config, value_loss_coef=1.0, kl_coef=0.0, final_kl_coef=0.0)
    val = np.asarray(value, dtype=F32).reshape(B, L)
    zeros = np.zeros((B, L - 1), dtype=F32)
    with np.errstate(all="ignore"):
        res = orl.token_loss(b, zeros, zeros, cfg, 0, 10, packed, value=val)
        adv = np.zeros((B, L), dtype=F32)
        adv[:, 1:] = (b["rewards"][:, 1:].astype(F32) - val[:, :-1]).astype(F32)
    stats = {k: float(res["stats"].get(k, 0.0)) for k in VALUE_STAT_KEYS}
    return adv.reshape(-1), res["g_value"].reshape(-1), stats


def columns(batch: dict) -> dict:
    """The witness's keyword arguments out of a batch dict."""
    return {k: batch[k] for k in ("labels", "rewards", "group_tokens", "num_labels", "overflow")}
