"""Per-token check of the token-level (PPO / REINFORCE) loss term (plain numpy; no kernel runs here).

Why: with `policy_loss` "ppo" (the GRPO default) or "reinforce" every number that trains the model comes out of
`grpo_loss_partial_kernel` (csrc/prl_loss.hip) and its per-token rule `prl_token_eval` (csrc/prl_token_math.h): g_nlp[u] =
d loss / d new_logprob, g_ent[u], the fp64 loss and 30 statistics.  The suite saw them through d logits of goldens under the 1e-4
max norm and through statistics held to `1e-4 max(|want|, 1)`, which for `kl` or `token_weight` (1e-3 .. 1e-5) allows more than
the value itself.  Here every token and every statistic is measured against the size of its own terms.

The witness (`witness`) restates oracle/rl_loss.py's ppo / reinforce branches (reference rl/__init__.py:238-439) and the comments of
csrc/prl_token_math.h for an unshifted batch - packed [1, T] or padded [B, L].  In fp32, exactly as the kernel forms them:

    lrno_u = new_u - old_u      lrrn_u = ref_u - new_u      (ref_u - old_u, which feeds the `ratio_ref_old` statistic only)
    w_u    = 1 / group_tokens_u  or  token_weight = 1 / batch_size;  then w_u * (1 - overflow_u) with overlong_filtering

(build.py compiles with `-O3 -ffp-contract=off` and nothing that relaxes division, so `1.0f / group_tokens` is the IEEE quotient
numpy forms - the argument of seq_term_checks.py).  Everything after that is fp64, with the loss config's fp32 clip_lo, clip_hi,
clamp_log_ratio_ref_new (C), kl_coef and entropy_coef:

    ratio = exp(lrno)  (inf above FLT_MAX, as expf)        A = adv or reward;  relu: A < 0 -> 0, NaN stays
    cl = clamp(lrrn, -C, C)    kl = e^cl - cl - 1    kl_inside = -C <= lrrn <= C    dkl = (1 - e^cl) kl_inside
    ppo:        s1 = ratio A,  s2 = clamp(ratio, lo, hi) A,  inside = lo <= ratio <= hi,  d1 = ratio A,  d2 = d1 inside
                pol, dpol = (s1, d1) if s1 < s2;  (s2, d2) if s2 < s1;  (s1, 0.5 d1 + 0.5 d2) on a tie;  NaN otherwise
    reinforce:  crr = clamp(ratio, 0, hi);  pol = new A crr;  dpol = A crr
    loss_t = pol - kl_coef kl [+ entropy_coef entropy]       v = loss_t w
    finite = v is finite in fp32 (|s1|, |pol|, |loss_t|, |v| <= FLT_MAX and not NaN: the one overflow the semantics depend on)
    contrib = nan_to_num(v)   g_nlp = -(dpol - kl_coef dkl) w if finite else 0   g_ent = -entropy_coef w if finite and the term is on

on the labelled, valid tokens: column >= 1 of every row, and - with `flat_micro_batches` - position_ids != 0.  Every decision
(inside / outside, s1 < s2, tie, finite) is taken from the fp64 values.  No token is left out of a comparison: instead the witness
REFUSES a case (`BadCase`) in which a labelled token's ratio lies within GUARD (relative) of a clip bound, or |ref - new| within
GUARD of C, without being exactly on it - there the decision would hang on fp32 rounding of expf and the case is badly built.

Metrics.  Per token (`check_tokens`): |got - want| / scale_u with the no-cancellation magnitude of the same expression,
scale_u = (|dpol| + |kl_coef| |1 - e^cl| kl_inside) |w| (|dpol| is one product: |A| ratio where the policy branch contributes, half
of it on a tie with the clipped side, |A| crr for reinforce); where scale_u == 0 - unlabelled tokens, column 0, a flat sequence
start, the clipped side, A = 0, overflow = 1 under filtering, non-finite tokens - got must be exactly 0.  g_ent is one product:
|got - want| / |want|, exactly 0 where want is.  Statistics (`check_stats`): sums as |got - want| / sum_u |term_u|, the loss as
|got - want| / sum_u |contrib_u|; the counts, the counters and max / min of reward, advantage and token weight (selections of fp32
inputs / of one IEEE quotient) exactly equal, NaN where a labelled value is NaN (torch's max / min); max_kl / min_kl under the
per-token metric, |got - want| / max_u (e^cl + |cl| + 1) - |max a - max b| <= max |a - b|.

Bounds.  None comes from a kernel.  TOKEN_BOUND / STAT_BOUND / LOSS_BOUND = 4 x the largest value of the same metric for the
oracle's own fp32 path (`oracle.rl_loss.token_loss`, pinned to the reference by the goldens) over every case of
tests/test_gpu_token_edges.py, measured on the CPU (TOKEN_REF, rounded up to two digits; tests/test_token_term_checks_host.py
re-measures it and fails if the oracle exceeds what is written; DESIGN.md section 7 holds the table).  4 x is the project's standing
margin: 1-2 ulp of the hardware expf, the reciprocal-multiply of the FAST path and a different summation order.  The measured
STAT_BOUND (numpy's pairwise fp32 sums, per sequence and then over sequences) separates the "every 64th token dropped" mutant
(1.6e-2) by two orders of magnitude, so the MEASURED statistic bound is the one in use, not the derived n_lane 2^-24 + 2^-23.
"""

from __future__ import annotations

import dataclasses

import numpy as np

import grad_checks as gc
from seq_term_checks import GUARD, BadCase, clip_bounds

F32 = np.float32
FLT_MAX = float(np.finfo(np.float32).max)

# the summed statistics in the order of the kernel's partial record (P_REWARD .. P_TW); all but the two ratio sums are per label
SUM_STATS = ("reward", "entropy", "old_logprobs", "new_logprobs", "ref_logprobs", "advantage", "kl", "kl_new_old",
             "mean_abs_log_ratio_new_old", "ratio_new_old", "ratio_new_old_sum", "ratio_new_old_squared_sum", "ratio_ref_new",
             "ratio_ref_old", "clamp_log_ratio_ref_new_indicator", "clamp_log_ratio_new_old_indicator", "token_weight")
EXACT_STATS = ("num_output_tokens_sum", "num_sequences", "max_reward", "min_reward", "max_advantage", "min_advantage",
               "max_token_weight", "min_token_weight", "nonfinite_new_logprobs", "nonfinite_log_ratio_ref_new", "nonfinite_kl",
               "bad_group_tokens")
KL_EXTREMES = ("max_kl", "min_kl")

# case of tests/test_gpu_token_edges.py -> (token, statistic, loss): the metrics of this module for the oracle's fp32 path against
# the witness, largest value over the case's loss configurations, measured on the CPU, rounded up to two digits
TOKEN_REF = {
    "branches": (1.8e-7, 1.2e-6, 1.2e-7),  # RATIOS x advantage > 0, < 0, 0.0, -0.0 x ref - new in {0, +-C, +-2C} exactly, 64 loss configurations
    "tie": (4.2e-7, 6.2e-8, 1.4e-8),  # epsilon 0, new == old: the ratio on both bounds
    "nonfinite": (3.2e-6, 3.1e-6, 1.9e-8),  # 290 ordinary tokens and one poisoned (the ordinary ones; a saturated sum is its own scale)
    "rounds": (7.0e-6, 1.3e-7, 1.1e-9),  # 4 199 427 tokens; the token value is the KL part 1 - e^cl at |cl| = 0.02, alone on the clipped side
    "padded": (7.1e-6, 2.3e-4, 6.0e-8),  # [B, L] down to L = 2: `kl_new_old` = ratio - log ratio - 1 of a handful of tokens, each good to 2^-24 / 4e-4
    "flat": (5.6e-6, 2.9e-6, 1.7e-9),  # 8195 tokens, 17 sequence starts
    "e2e": (9.0e-8, 9.9e-7, 1.5e-8),  # the `branches` table on the log-probs of a V = 1031 model
}
TOKEN_BOUND = 4.0 * max(v[0] for v in TOKEN_REF.values())
STAT_BOUND = 4.0 * max(v[1] for v in TOKEN_REF.values())
LOSS_BOUND = 4.0 * max(v[2] for v in TOKEN_REF.values())
assert TOKEN_BOUND < gc.MUTANT_FLOOR  # "g_nlp x 1.001" scores 1e-3
assert STAT_BOUND < 1.0 / 64 / 4      # "every 64th labelled token dropped" scores ~1/64


def config_scalars(config: dict) -> dict:
    """The fp32 scalars `make_loss_config` hands the kernels at a step where kl_coef / entropy_bonus equal their final values."""
    assert config.get("kl_coef", 0.1) == config.get("final_kl_coef", 0.1)
    assert config.get("entropy_bonus", 0.0) == config.get("final_entropy_bonus", 0.0)
    lo, hi = clip_bounds(config)
    bs = config.get("batch_size", 0)
    return dict(lo=lo, hi=hi, C=float(F32(config.get("clamp_log_ratio_ref_new_value", 10))), kl_coef=float(F32(config.get("kl_coef", 0.1))),
                ent_coef=float(F32(config.get("entropy_bonus", 0.0))), use_entropy=config.get("entropy_bonus", 0.0) != 0.0,
                token_weight=(F32(1) / F32(bs)) if bs else F32(np.inf))


@dataclasses.dataclass
class Witness:
    shape: tuple
    valid: np.ndarray       # [N] bool: a shifted position exists (column >= 1; not a flat sequence start)
    mask: np.ndarray        # [N] bool: valid and labelled
    finite: np.ndarray      # [N] bool: fp32 loss_t * w is finite (meaningful on `mask`)
    g_nlp: np.ndarray       # [N] fp64, 0 off `mask`
    g_ent: np.ndarray
    scale: np.ndarray       # [N] fp64: the no-cancellation magnitude of g_nlp, 0 off `mask`
    contrib: np.ndarray     # [N] fp64: nan_to_num(loss_t * w), 0 off `mask`
    terms: np.ndarray       # [17, N] fp64: what each token adds to the statistics of SUM_STATS, 0 off `mask`
    kl_scale: float         # max over `mask` of e^cl + |cl| + 1
    loss: float
    loss_scale: float       # sum |contrib|
    stats: dict             # name -> value: SUM_STATS, EXACT_STATS, KL_EXTREMES, "loss"
    stat_scale: dict        # name -> sum |term| for SUM_STATS
    ratio: np.ndarray       # [N] fp64
    lrrn: np.ndarray        # [N] fp64 of the fp32 difference


def _flat(a, dtype=F32):
    return np.ascontiguousarray(np.asarray(a), dtype=dtype).reshape(-1)


def _nan_to_num(x):
    return np.where(np.isnan(x), 0.0, np.clip(x, -FLT_MAX, FLT_MAX))


def _overflows(x):
    """True where a finite-or-not fp64 value is not a finite fp32 one."""
    return ~(np.abs(x) <= FLT_MAX)


def _guard(what, x, bound, mask):
    near = mask & (np.abs(x - bound) <= GUARD * abs(bound)) & (x != bound)
    if near.any():
        u = int(np.flatnonzero(near)[0])
        raise BadCase(f"token {u}: {what} {x[u]!r} is within {GUARD:g} of the bound {bound!r} without being on it")


def witness(config: dict, labels, new_logprobs, entropy, old_logprobs, ref_logprobs, advantages, rewards, group_tokens, num_labels,
            overflow, position_ids=None, flat: bool = False, guard: bool = True, mutate: str | None = None) -> Witness:
    """The fp64 witness of the module docstring.  `labels` [B, L]; the other columns the same shape, token-aligned (column 0 of
    `new_logprobs` / `entropy` unused).  `position_ids`: given for a packed [1, T] batch (sequence starts are counted);
    `flat`: `flat_micro_batches`.  `mutate`: a WRONG rule, for the host test's mutants - "strict_inside" (lo < ratio < hi),
    "clipped_grad" (d2 = d1 outside the range), "kl_outside" (the KL gradient kept outside +-C), "no_relu", "no_overflow"."""
    lab = np.asarray(labels)
    B, L = lab.shape
    N = B * L
    c = config_scalars(config)
    new, ent, old, ref = _flat(new_logprobs), _flat(entropy), _flat(old_logprobs), _flat(ref_logprobs)
    adv, rew, gt, nl, ovf = _flat(advantages), _flat(rewards), _flat(group_tokens), _flat(num_labels), _flat(overflow)
    assert all(a.size == N for a in (new, ent, old, ref, adv, rew, gt, nl, ovf))
    col = np.tile(np.arange(L), B)
    valid = col != 0
    packed = B == 1 and position_ids is not None
    if packed:
        pos = _flat(position_ids, np.int64)
        starts = pos == 0
        starts[0] = True
        num_sequences = int(starts.sum())
        if flat:
            valid &= pos != 0
    else:
        assert not flat
        num_sequences = B
    mask = valid & (lab.reshape(-1) != -100)
    gn = bool(config.get("group_normalization", False))
    with np.errstate(all="ignore"):
        lrno32, lrrn32, lrro32 = (new - old).astype(F32), (ref - new).astype(F32), (ref - old).astype(F32)
        w32 = (F32(1) / gt).astype(F32) if gn else np.full(N, c["token_weight"], dtype=F32)
        if config.get("overlong_filtering", False) and mutate != "no_overflow":
            w32 = (w32 * (F32(1) - ovf)).astype(F32)
        lrno, lrrn, w = lrno32.astype(np.float64), lrrn32.astype(np.float64), w32.astype(np.float64)
        ratio = np.exp(lrno)
        ratio = np.where(ratio > FLT_MAX, np.inf, ratio)
        A32 = adv if config.get("use_advantages", True) else rew
        A = A32.astype(np.float64)
        if config.get("relu_log_p_weights", False) and mutate != "no_relu":
            A = np.where(A < 0, 0.0, A)
        C, lo, hi = c["C"], c["lo"], c["hi"]
        cl = np.where(np.isnan(lrrn), lrrn, np.clip(lrrn, -C, C))
        ecl = np.exp(cl)
        kl = ecl - cl - 1.0
        kl_no = ratio - lrno - 1.0
        kl_inside = (lrrn >= -C) & (lrrn <= C)
        algo = config.get("policy_loss", "ppo")
        if guard:
            if algo == "ppo":
                _guard("ratio", ratio, lo, mask)
            _guard("ratio", ratio, hi, mask)
            _guard("|ref - new|", np.abs(lrrn), C, mask)
        if algo == "ppo":
            cr = np.where(np.isnan(ratio), ratio, np.clip(ratio, lo, hi))
            s1, s2 = ratio * A, cr * A
            clamp_no = (cr != ratio).astype(np.float64)
            inside = ((ratio > lo) & (ratio < hi)) if mutate == "strict_inside" else ((ratio >= lo) & (ratio <= hi))
            d1 = ratio * A
            d2 = d1 if mutate == "clipped_grad" else np.where(inside, d1, 0.0)
            nan = np.isnan(s1) | np.isnan(s2)
            pol = np.where(nan, np.nan, np.where(s1 < s2, s1, np.where(s2 < s1, s2, s1)))
            dpol = np.where(nan, np.nan, np.where(s1 < s2, d1, np.where(s2 < s1, d2, 0.5 * d1 + 0.5 * d2)))
            pscale = np.where(s1 < s2, np.abs(d1), np.where(s2 < s1, np.abs(d2), 0.5 * np.abs(d1) + 0.5 * np.abs(d2)))
            ratio_stat = ratio
            over = np.zeros(N, dtype=bool)  # an overflowing s1 / s2 is +-inf in fp32 and decides the same way; only the chosen one counts
        elif algo == "reinforce":
            clamp_no = (ratio > hi).astype(np.float64)
            crr = np.where(np.isnan(ratio), ratio, np.clip(ratio, 0.0, hi))
            pol = new.astype(np.float64) * A * crr
            dpol = A * crr
            pscale = np.abs(dpol)
            ratio_stat = crr
            over = np.zeros(N, dtype=bool)
        else:
            raise ValueError(f"the token-level witness covers ppo and reinforce, not {algo!r}")
        loss_t = pol - c["kl_coef"] * kl
        over |= _overflows(pol) | _overflows(loss_t)
        if c["use_entropy"]:
            loss_t = loss_t + c["ent_coef"] * ent.astype(np.float64)
            over |= _overflows(loss_t)
        v = loss_t * w
        finite = ~(over | _overflows(v))
        contrib = np.where(mask, _nan_to_num(np.where(over & ~np.isnan(v), np.sign(v) * np.inf, v)), 0.0)
        dkl = (1.0 - ecl) if mutate == "kl_outside" else np.where(kl_inside, 1.0 - ecl, 0.0)
        live = mask & finite
        g_nlp = np.where(live, -((dpol - c["kl_coef"] * dkl) * w), 0.0)
        scale = np.where(live, (pscale + abs(c["kl_coef"]) * np.abs(dkl)) * np.abs(w), 0.0)
        scale = np.where(np.isnan(scale), 0.0, scale)
        g_ent = np.where(live & c["use_entropy"], -(c["ent_coef"] * w), 0.0)
        # statistics: nan_to_num(x / num_labels) in fp32 on the labelled tokens
        nl64 = nl.astype(np.float64)
        f32v = lambda x: np.where(np.abs(x) > FLT_MAX, np.sign(x) * np.inf, x)  # noqa: E731 - the fp32 value of a statistic's input
        per = lambda x: np.where(mask, _nan_to_num(f32v(f32v(x) / nl64)), 0.0)  # noqa: E731
        raw = lambda x: np.where(mask, _nan_to_num(f32v(x)), 0.0)  # noqa: E731
        terms = np.stack([
            per(rew.astype(np.float64)), per(ent.astype(np.float64)), per(old.astype(np.float64)), per(new.astype(np.float64)),
            per(ref.astype(np.float64)), per(adv.astype(np.float64)), per(kl), per(kl_no), per(np.abs(lrno)), per(ratio_stat),
            raw(ratio_stat), raw(f32v(ratio_stat) * f32v(ratio_stat)), per(np.exp(lrrn)), per(np.exp(lrro32.astype(np.float64))),
            per((np.abs(lrrn) > C).astype(np.float64)), per(clamp_no), per(w)])
        kl_scale = float((ecl + np.abs(cl) + 1.0)[mask].max()) if mask.any() else 0.0

    def extreme(x32, fn, empty):
        sel = x32[mask]
        return float(fn(sel)) if sel.size else empty  # numpy's max / min return NaN if any element is NaN, like torch's

    stats = {k: float(terms[i].sum()) for i, k in enumerate(SUM_STATS)}
    stat_scale = {k: float(np.abs(terms[i]).sum()) for i, k in enumerate(SUM_STATS)}
    with np.errstate(all="ignore"):
        bad_kl = np.isnan(kl) | _overflows(kl)
        stats.update(
            loss=-float(contrib.sum()), num_output_tokens_sum=float(mask.sum()), num_sequences=float(num_sequences),
            max_reward=extreme(rew, np.max, -np.inf), min_reward=extreme(rew, np.min, np.inf),
            max_advantage=extreme(adv, np.max, -np.inf), min_advantage=extreme(adv, np.min, np.inf),
            max_token_weight=extreme(w32, np.max, -np.inf), min_token_weight=extreme(w32, np.min, np.inf),
            max_kl=extreme(kl, np.max, -np.inf), min_kl=extreme(kl, np.min, np.inf),
            nonfinite_new_logprobs=float((valid & ~np.isfinite(new)).sum()), nonfinite_log_ratio_ref_new=float((valid & ~np.isfinite(lrrn32)).sum()),
            nonfinite_kl=float((valid & bad_kl).sum()), bad_group_tokens=float((valid & ~(gt > 0)).sum()) if gn else 0.0)
    return Witness((B, L), valid, mask, finite, g_nlp, g_ent, scale, contrib, terms, kl_scale, stats["loss"], float(np.abs(contrib).sum()),
                   stats, stat_scale, ratio, lrrn)


# ---- metrics ------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class TokenCheck:
    err: float              # max over tokens with scale > 0 of |got - want| / scale
    at: int                 # flat index of it
    got: float
    want: float
    ent_err: float          # max over tokens with want != 0 of |got - want| / |want| for g_ent
    ent_at: int
    stray: int              # tokens whose g_nlp or g_ent must be exactly 0 and is not (NaN included; must be 0)
    stray_at: int | None

    def ok(self, bound: float | None = None) -> bool:
        bound = TOKEN_BOUND if bound is None else bound
        return self.stray == 0 and self.err <= bound and self.ent_err <= bound

    def __str__(self):
        s = (f"g_nlp error {self.err:.3e} at token {self.at} (got {self.got:.9e} want {self.want:.9e}); g_ent error {self.ent_err:.3e} at token "
             f"{self.ent_at}")
        if self.stray:
            s += f"; {self.stray} tokens must be exactly 0 and are not, first {self.stray_at}"
        return s


def _rel(got, want, scale):
    live = scale > 0
    with np.errstate(all="ignore"):
        rel = np.where(live, np.abs(got - want) / np.where(live, scale, 1.0), 0.0)
    rel = np.where(np.isnan(rel), np.inf, rel)
    bad = ~live & ~(got == 0)  # NaN == 0 is false: a NaN counts
    return rel, bad


def check_tokens(got_g_nlp, got_g_ent, w: Witness) -> TokenCheck:
    """The per-token metric of the module docstring.  `got_g_ent` None: no entropy gradient was delivered (the term is off)."""
    g = np.asarray(got_g_nlp, dtype=np.float64).reshape(-1)
    assert g.shape == w.g_nlp.shape
    rel, bad = _rel(g, w.g_nlp, w.scale)
    if got_g_ent is None:
        assert not w.g_ent.any()
        erel, ebad = np.zeros_like(rel), np.zeros_like(bad)
    else:
        e = np.asarray(got_g_ent, dtype=np.float64).reshape(-1)
        erel, ebad = _rel(e, w.g_ent, np.abs(w.g_ent))
    bad = bad | ebad
    u, ue = (int(rel.argmax()), int(erel.argmax())) if rel.size else (0, 0)
    return TokenCheck(float(rel[u]) if rel.size else 0.0, u, float(g[u]) if rel.size else 0.0, float(w.g_nlp[u]) if rel.size else 0.0,
                      float(erel[ue]) if rel.size else 0.0, ue, int(bad.sum()), int(np.flatnonzero(bad)[0]) if bad.any() else None)


@dataclasses.dataclass
class StatCheck:
    err: float              # max over SUM_STATS of |got - want| / sum |term|
    name: str
    loss_err: float         # |got - want| / sum |contrib|
    kl_err: float           # max over max_kl / min_kl of |got - want| / kl_scale
    mismatch: list          # names of the exactly compared statistics that differ, of sums that must be exactly 0 and are not

    def ok(self, stat_bound: float | None = None, loss_bound: float | None = None, token_bound: float | None = None) -> bool:
        return (not self.mismatch and self.err <= (STAT_BOUND if stat_bound is None else stat_bound)
                and self.loss_err <= (LOSS_BOUND if loss_bound is None else loss_bound)
                and self.kl_err <= (TOKEN_BOUND if token_bound is None else token_bound))

    def __str__(self):
        s = f"statistics {self.err:.3e} ({self.name}); loss {self.loss_err:.3e}; max / min kl {self.kl_err:.3e}"
        return s + (f"; differ where they must be equal: {self.mismatch}" if self.mismatch else "")


def _same(a: float, b: float) -> bool:
    return a == b or (np.isnan(a) and np.isnan(b))


def check_stats(got: dict, w: Witness) -> StatCheck:
    """The statistic metric of the module docstring.  `got`: name -> value; a name it does not hold is not checked (the oracle has
    no counters)."""
    worst, name, mismatch = 0.0, "-", []
    for k in SUM_STATS:
        if k not in got:
            continue
        g, want, sc = float(got[k]), w.stats[k], w.stat_scale[k]
        if sc == 0:
            if g != 0:
                mismatch.append(k)
            continue
        e = abs(g - want) / sc
        e = np.inf if np.isnan(e) else e
        if e > worst:
            worst, name = e, k
    for k in EXACT_STATS:
        if k in got and not _same(float(got[k]), w.stats[k]):
            mismatch.append(k)
    kl_err = 0.0
    for k in KL_EXTREMES:
        if k not in got:
            continue
        g, want = float(got[k]), w.stats[k]
        if np.isinf(want) or np.isnan(want) or w.kl_scale == 0:
            if not _same(g, want):
                mismatch.append(k)
            continue
        e = abs(g - want) / w.kl_scale
        kl_err = max(kl_err, np.inf if np.isnan(e) else e)
    loss_err = 0.0
    if "loss" in got:
        g = float(got["loss"])
        if w.loss_scale == 0:
            loss_err = 0.0 if g == 0 else np.inf
        else:
            loss_err = abs(g - w.loss) / w.loss_scale
            loss_err = np.inf if np.isnan(loss_err) else loss_err
    return StatCheck(float(worst), name, float(loss_err), float(kl_err), mismatch)


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=F32).reshape(-1).view(np.uint32)


def n_bit_differences(a, b) -> tuple[int, int | None]:
    """(number of fp32 entries that are not BIT-equal, first such index)."""
    d = bits(a) != bits(b)
    return int(d.sum()), (int(np.flatnonzero(d)[0]) if d.any() else None)


# ---- the oracle's own fp32 path on the same arrays (the yardstick of every bound) ---------------------------------------
def oracle_fp32(config: dict, batch: dict, flat: bool = False):
    """`oracle.rl_loss.token_loss` on an unshifted batch of this module's layout -> (g_nlp [N], g_ent [N] fp32 token-aligned, stats
    dict with "loss").  `flat`: the oracle knows no flat micro-batches; a sequence start that is no valid position is the same as
    an unlabelled one to every sum, so its label is set to -100."""
    from oracle import rl_loss as orl

    b = dict(batch)
    packed = b["labels"].shape[0] == 1 and b.get("position_ids") is not None
    if flat:
        lab = b["labels"].copy()
        lab[b["position_ids"] == 0] = -100
        b["labels"] = lab
    b.setdefault("input_ids", np.zeros_like(b["labels"]))
    res = orl.token_loss(b, b["new_logprobs"][:, 1:], b["entropy"][:, 1:], config, 0, 10, packed)
    B, L = b["labels"].shape
    g, gh = np.zeros((B, L), dtype=F32), np.zeros((B, L), dtype=F32)
    g[:, 1:], gh[:, 1:] = res["g_nlp"], res["g_ent"]
    stats = {k: v for k, v in res["stats"].items() if k in SUM_STATS + KL_EXTREMES + EXACT_STATS}
    stats["loss"] = float(res["loss"])
    stats["num_sequences"] = float(res["num_sequences"])
    if "num_output_tokens_sum" not in stats:  # the no-label dict
        stats["num_output_tokens_sum"] = 0.0
    return g.reshape(-1), gh.reshape(-1), stats


def columns(batch: dict, packed_positions: bool = True) -> dict:
    """The witness's keyword arguments out of a batch dict."""
    kw = {k: batch[k] for k in ("labels", "new_logprobs", "entropy", "old_logprobs", "ref_logprobs", "advantages", "rewards", "group_tokens",
                                "num_labels", "overflow")}
    if packed_positions and batch["labels"].shape[0] == 1 and batch.get("position_ids") is not None:
        kw["position_ids"] = batch["position_ids"]
    return kw
