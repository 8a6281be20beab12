"""Per-segment check of the sequence-level (GSPO) policy term (plain numpy; no kernel runs here).

Why: with `policy_loss="gspo"` every number that trains the model is one clipped ratio and one gradient coefficient per
SEQUENCE, copied onto the sequence's tokens.  The suite judged them through d logits under `helpers.rel_err`
(`max|got - want| / max|want|` at 1e-4): a token credited to the neighbouring segment moves one sequence's mean log-ratio by
1/n of one token's log-ratio (1e-6 relative on an 8192-token segment), and a coefficient wrong by 1.001 on a short segment
hides behind the maximum over all rows.  Here every segment is measured on its own.

The witness (`witness`) restates oracle/rl_loss.py's `gspo` branch (reference rl/__init__.py:310-352, rl/utils.py:106-208)
and the comments of csrc/prl_loss.hip.  Per token, in fp32 exactly as the kernel forms them:

    lr_u = new_u - old_u                                  one fp32 subtraction
    w_u  = 1 / group_tokens_u  or  1 / batch_size         fp32 division; then w_u * (1 - overflow_u) with overlong_filtering

over the labelled tokens u >= 1 of segment s (column 0 predicts nothing).  Everything after that is fp64:

    sums[0..3, s] = sum lr_u, sum adv_u, count, sum w_u
    den   = max(count, 1e-6)       ratio = exp(sums[0] / den)      A = sums[1] / den       valid = count > 0 and sums[3] > 0
    s1 = ratio A,  s2 = clip(ratio, lo, hi) A,  inside = lo <= ratio <= hi        (lo, hi: the fp32 values of the loss config)
    dmin  = A if s1 < s2;  A inside if s2 < s1;  0.5 A + 0.5 A inside on a tie    (torch.min's tie rule, clamp's inclusive rule)
    coef  = -(sums[3] valid) dmin ratio / den grad_scale           (0 with zero_out)
    ind   = clip(ratio) != ratio and valid
    loss  = -sum_s min(s1, s2) valid sums[3]                        (0 with zero_out)
    ext_g[u] = coef[clamp(seg[u], 0, S - 1)]        ext_c[u] = ind[clamp(seg[u] - seg[0], 0, S - 1)]

Metric (`check_terms`): `coef` per segment as |got - want| / |want| - one product, no cancellation; where want == 0
(invalid segment, zero mean advantage, the clipped side without gradient, zero_out) got must be exactly 0; where want is
NaN got must be NaN.  `indicator` exactly equal.  Loss as |got - want| / sum_s |min(s1, s2) valid sums[3]|.  No segment is
left out: instead the witness REFUSES a case (`BadCase`) in which some segment's fp64 ratio lies within 1e-4 relative of a
clip bound without being exactly on it - there the clip decision would hang on fp32 rounding and the case is badly built.

Bounds.  COEF_BOUND / LOSS_BOUND = 4 x the largest value of the same metric for the oracle's own fp32 GSPO branch
(`oracle.rl_loss.token_loss`, pinned to the reference by the goldens; sequential fp32 sums) over every case of
tests/test_gpu_gspo_edges.py, measured on the CPU (SEQ_REF, rounded up to two digits; tests/test_seq_term_checks_host.py
re-measures it and fails if the oracle exceeds what is written; DESIGN.md section 7 holds the table).  4 x for a different
summation order and 1-2 ulp of the hardware expf, the margin of grad_checks.  No bound comes from a kernel.

The sums bound is derived (`check_sums`): fp64 sums of fp32 terms, so only the order differs:
|got - want| <= n_s 2^-52 sum|terms| per segment and column; the count exactly equal.  The weight column stays on the same
bound: pipelinerl_amd/build.py compiles with `-O3 -ffp-contract=off` and nothing that relaxes division (no -ffast-math, no
approximate reciprocal, and hipcc's default is the correctly rounded fp32 division), so `1.0f / group_tokens` is the IEEE
quotient numpy forms.
"""

from __future__ import annotations

import dataclasses

import numpy as np

import grad_checks as gc

F32 = np.float32
GUARD = 1e-4            # a ratio closer than this (relative) to a clip bound, and not on it, makes a case badly built
EPS52 = 2.0 ** -52

# case of tests/test_gpu_gspo_edges.py -> (coef, loss): the metric of this module for the oracle's fp32 GSPO branch against
# the witness, largest value over the case's loss configurations, measured on the CPU, rounded up to two digits
SEQ_REF = {
    "geometry": (4.1e-5, 1.8e-5),  # runs of 1 .. 8192 tokens x the four weight configurations; the 8192-token segment under group normalization: 8192 sequential fp32 additions of 1 / group_tokens
    "many": (2.3e-7, 4.1e-9),  # 700 segments of 1 .. 5 tokens
    "wide": (2.9e-6, 2.2e-8),  # 300 segments over 1.26 M columns
    "clip": (3.8e-7, 2.6e-7),  # ratios 0.90 .. 1.10 x advantage > 0, < 0, = 0
    "tie": (3.5e-6, 3.3e-6),  # epsilon 0, new == old: the ratio on both bounds
    "slice": (3.9e-7, 1.3e-7),  # ids from 3, pre-reduced sums, grad_scale 2
    "nan": (2.4e-7, 0.0),  # one NaN log-prob (its segment aside)
    "e2e": (2.8e-7, 1.8e-8),  # the first 2048 tokens of `geometry`, log-probs of a V = 1031 model
}
COEF_BOUND = 4.0 * max(v[0] for v in SEQ_REF.values())
LOSS_BOUND = 4.0 * max(v[1] for v in SEQ_REF.values())
assert COEF_BOUND < gc.MUTANT_FLOOR  # "coef x 1.001" scores 1e-3


class BadCase(ValueError):
    """A case whose clip decision depends on fp32 rounding."""


def clip_bounds(config: dict) -> tuple[float, float]:
    """(clip_lo, clip_hi) as the loss config holds them: combined in double, stored as fp32 (make_loss_config)."""
    return float(F32(1 - config.get("epsilon_low", 0.2))), float(F32(1 + config.get("epsilon_high", 0.2)))


def token_terms(config: dict, labels, new_logprobs, old_logprobs, advantages, group_tokens, overflow):
    """(mask [T], terms [4, T] fp64): the per-token inputs of the four sums, formed in fp32 as the kernel forms them."""
    lab = np.asarray(labels).reshape(-1)
    f = lambda a: np.asarray(a, dtype=F32).reshape(-1)  # noqa: E731
    new, old, adv, gt, ovf = f(new_logprobs), f(old_logprobs), f(advantages), f(group_tokens), f(overflow)
    mask = lab != -100
    mask[0] = False
    with np.errstate(all="ignore"):
        lr = (new - old).astype(F32)
        if config.get("group_normalization", False):
            w = (F32(1) / gt).astype(F32)
        else:
            w = np.full(lab.shape, F32(1) / F32(config["batch_size"]), dtype=F32)
        if config.get("overlong_filtering", False):
            w = (w * (F32(1) - ovf)).astype(F32)
    return mask, np.stack([lr.astype(np.float64), adv.astype(np.float64), np.ones(lab.shape), w.astype(np.float64)])


@dataclasses.dataclass
class Witness:
    sums: np.ndarray        # [4, S] fp64: log-ratio, advantage, count, weight (the kernel's row order)
    abs_sums: np.ndarray    # [4, S] sum of |terms| (the size the sums bound is taken from); zeros when `sums` was supplied
    ratio: np.ndarray       # [S]
    coef: np.ndarray        # [S] fp64
    indicator: np.ndarray   # [S] 0.0 / 1.0
    valid: np.ndarray       # [S] bool
    loss: float
    loss_scale: float       # sum_s |min(s1, s2) valid w_sum|
    ext_g: np.ndarray       # [T] fp64
    ext_c: np.ndarray       # [T]
    lo: float
    hi: float


def segment_sums(seg, mask, terms, n_segments: int):
    """fp64 (sums, sums of absolute values) [4, S] of the labelled tokens; an id outside [0, S) on a labelled token raises."""
    ids = np.asarray(seg).reshape(-1)[mask]
    if ids.size and (ids.min() < 0 or ids.max() >= n_segments):
        raise BadCase("a labelled token carries a segment id outside [0, n_segments)")
    sums, abs_sums = np.zeros((4, n_segments)), np.zeros((4, n_segments))
    for k in range(4):
        sums[k] = np.bincount(ids, weights=terms[k][mask], minlength=n_segments)
        abs_sums[k] = np.bincount(ids, weights=np.abs(terms[k][mask]), minlength=n_segments)
    return sums, abs_sums


def expand(seg, coef, indicator):
    """The per-token rule: (coef[clamp(seg, 0, S - 1)], indicator[clamp(seg - seg[0], 0, S - 1)]), dtype of the inputs."""
    seg = np.asarray(seg).reshape(-1)
    top = max(len(coef) - 1, 0)
    return np.asarray(coef)[np.clip(seg, 0, top)], np.asarray(indicator)[np.clip(seg - seg[0], 0, top)]


def segment_terms(config: dict, sums, grad_scale: float = 1.0, zero_out: bool = False, strict_inside: bool = False, guard: bool = True):
    """fp64 (ratio, coef, indicator, valid, loss, loss_scale) of per-segment sums [4, S].  `strict_inside`: the WRONG inside
    rule lo < ratio < hi (what the host test's mutant applies).  `guard`: refuse a ratio that nearly touches a clip bound."""
    lo, hi = clip_bounds(config)
    sums = np.asarray(sums, dtype=np.float64)
    with np.errstate(all="ignore"):
        cnt, w_sum = sums[2], sums[3]
        den = np.maximum(cnt, 1e-6)
        ratio = np.exp(sums[0] / den)
        adv = sums[1] / den
        if guard:
            for b in (lo, hi):
                near = (np.abs(ratio - b) <= GUARD * b) & (ratio != b)
                if near.any():
                    s = int(np.flatnonzero(near)[0])
                    raise BadCase(f"segment {s}: ratio {ratio[s]!r} is within {GUARD:g} of the clip bound {b!r} without being on it")
        valid = (cnt > 0) & (w_sum > 0)
        clipped = np.clip(ratio, lo, hi)
        s1, s2 = ratio * adv, clipped * adv
        inside = ((ratio > lo) & (ratio < hi)) if strict_inside else ((ratio >= lo) & (ratio <= hi))
        a_in = np.where(inside, adv, 0.0)
        dmin = np.where(s1 < s2, adv, np.where(s2 < s1, a_in, 0.5 * adv + 0.5 * a_in))
        dmin = np.where(np.isnan(s1) | np.isnan(s2), s1 + s2, dmin)
        wv = np.where(valid, w_sum, 0.0)
        coef = -wv * dmin * ratio / den * grad_scale
        part = np.minimum(s1, s2) * wv
        indicator = ((clipped != ratio) & valid).astype(np.float64)
        loss, loss_scale = -float(part.sum()), float(np.abs(part).sum())
    if zero_out:
        coef, loss = np.zeros_like(coef), 0.0
    return ratio, coef, indicator, valid, loss, loss_scale


def witness(config: dict, segment_ids, labels, new_logprobs, old_logprobs, advantages, group_tokens, overflow, *,
            n_segments: int | None = None, grad_scale: float = 1.0, zero_out: bool = False, sums=None, guard: bool = True) -> Witness:
    """The fp64 witness of the module docstring for the unshifted [1, T] columns of one packed row (or one slice of it).
    `sums` [4, S]: pre-reduced sums (as after the all-reduce over a sequence-parallel group) instead of the row's own."""
    seg = np.asarray(segment_ids).reshape(-1)
    S = int(seg.max()) + 1 if n_segments is None else int(n_segments)
    if sums is None:
        mask, terms = token_terms(config, labels, new_logprobs, old_logprobs, advantages, group_tokens, overflow)
        sums, abs_sums = segment_sums(seg, mask, terms, S)
    else:
        sums = np.asarray(sums, dtype=np.float64)
        assert sums.shape == (4, S)
        abs_sums = np.zeros_like(sums)
    ratio, coef, indicator, valid, loss, loss_scale = segment_terms(config, sums, grad_scale, zero_out, guard=guard)
    ext_g, ext_c = expand(seg, coef, indicator)
    lo, hi = clip_bounds(config)
    return Witness(sums, abs_sums, ratio, coef, indicator, valid, loss, loss_scale, ext_g, ext_c, lo, hi)


# ---- metrics ------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class SumsCheck:
    worst: float            # largest |got - want| / (n_s 2^-52 sum|terms|) over segments and the three summed columns (<= 1 passes)
    at: tuple               # (column, segment) of it
    count_mismatch: int     # segments whose count differs (must be 0)
    stray: int              # non-zero (or NaN) sums where no term exists (must be 0)

    def ok(self) -> bool:
        return self.count_mismatch == 0 and self.stray == 0 and self.worst <= 1.0

    def __str__(self):
        return (f"sums: worst |got - want| = {self.worst:.3g} x (n 2^-52 sum|terms|) at column {self.at[0]} segment {self.at[1]}; "
                f"{self.count_mismatch} counts differ; {self.stray} non-zero sums without a term")


def check_sums(got, w: Witness) -> SumsCheck:
    """The derived bound of the module docstring.  `got` [4, S] fp64."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == w.sums.shape
    n = w.sums[2]
    mismatch = int((got[2] != n).sum())
    worst, at, stray = 0.0, (0, 0), 0
    for k in (0, 1, 3):
        allow = n * EPS52 * w.abs_sums[k]
        diff = np.abs(got[k] - w.sums[k])
        dead = allow == 0
        stray += int((dead & ~(got[k] == w.sums[k])).sum())  # NaN == x is false: a NaN counts
        with np.errstate(all="ignore"):
            rel = np.where(dead, 0.0, diff / np.where(dead, 1.0, allow))
        rel = np.where(np.isnan(rel), np.inf, rel)
        if rel.size and rel.max() > worst:
            worst, at = float(rel.max()), (k, int(rel.argmax()))
    return SumsCheck(worst, at, mismatch, stray)


@dataclasses.dataclass
class TermsCheck:
    coef_err: float         # max over segments with want != 0 of |got - want| / |want|
    coef_seg: int
    coef_got: float
    coef_want: float
    stray: int              # segments where want == 0 and got != 0, or want is NaN and got is not (must be 0)
    stray_seg: int | None
    indicator_mismatch: int  # segments whose indicator differs (must be 0)
    loss_err: float         # |got - want| / sum_s |min(s1, s2) valid w_sum|; 0 when both are NaN or both exactly 0
    loss_got: float
    loss_want: float

    def ok(self, coef_bound: float = COEF_BOUND, loss_bound: float = LOSS_BOUND) -> bool:
        return self.stray == 0 and self.indicator_mismatch == 0 and self.coef_err <= coef_bound and self.loss_err <= loss_bound

    def __str__(self):
        s = (f"coef error {self.coef_err:.3e} at segment {self.coef_seg} (got {self.coef_got:.9e} want {self.coef_want:.9e}); "
             f"loss error {self.loss_err:.3e} (got {self.loss_got:.9e} want {self.loss_want:.9e}); "
             f"{self.indicator_mismatch} indicators differ")
        if self.stray:
            s += f"; {self.stray} segments must be exactly 0 (or NaN) and are not, first {self.stray_seg}"
        return s


def check_terms(got_coef, got_indicator, got_loss, w: Witness) -> TermsCheck:
    """The per-segment metric of the module docstring against a witness built with the same grad_scale / zero_out."""
    got = np.asarray(got_coef, dtype=np.float64).reshape(-1)
    ind = np.asarray(got_indicator, dtype=np.float64).reshape(-1)
    want = w.coef
    assert got.shape == want.shape and ind.shape == want.shape
    nan = np.isnan(want)
    zero = want == 0
    bad = (zero & ~(got == 0)) | (nan & ~np.isnan(got))
    live = ~zero & ~nan
    with np.errstate(all="ignore"):
        rel = np.where(live, np.abs(got - want) / np.where(live, np.abs(want), 1.0), 0.0)
    rel = np.where(np.isnan(rel), np.inf, rel)
    s = int(rel.argmax()) if rel.size else 0
    got_loss = float(got_loss)
    if np.isnan(w.loss):
        loss_err = 0.0 if np.isnan(got_loss) else float("inf")
    elif w.loss_scale == 0:
        loss_err = 0.0 if got_loss == 0 else float("inf")
    else:
        loss_err = abs(got_loss - w.loss) / w.loss_scale
        loss_err = float("inf") if np.isnan(loss_err) else loss_err
    return TermsCheck(float(rel[s]) if rel.size else 0.0, s, float(got[s]) if rel.size else 0.0, float(want[s]) if rel.size else 0.0,
                      int(bad.sum()), int(np.flatnonzero(bad)[0]) if bad.any() else None, int((ind != w.indicator).sum()),
                      loss_err, got_loss, w.loss)


def _bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=F32).reshape(-1).view(np.uint32)


def check_tokens(got_g, got_c, segment_ids, coef32, indicator32) -> tuple[int, int | None]:
    """(number of tokens whose `ext_g` or `ext_c` is not BIT-equal to the per-token rule applied to the fp32 `coef32` /
    `indicator32` the tokens were expanded from, first such column)."""
    want_g, want_c = expand(segment_ids, np.asarray(coef32, dtype=F32), np.asarray(indicator32, dtype=F32))
    bad = (_bits(got_g) != _bits(want_g)) | (_bits(got_c) != _bits(want_c))
    return int(bad.sum()), (int(np.flatnonzero(bad)[0]) if bad.any() else None)
