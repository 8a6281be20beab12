"""Per-entry check of the fused head's d hidden and d W (plain torch / numpy; no kernel runs here).  Built on
tests/grad_checks.py: the d logits witness and the size of its terms come from there and are carried through the two
products of the head's backward.

For hidden `h` [R, H] (bf16, exact), weight `W` [V, H] as stored, labels, token gradients g, gH and temperature:

    logits64          = h.double() @ W.double().T
    want_dl, scale_dl = grad_checks._witness_block(logits64, ...)        fp64 closed form, and its terms in absolute value
    want_dH = want_dl   @ W          scale_dH = scale_dl   @ |W|          flush_dH = flush_dl   @ |W| + F32_TINY
    want_dW = want_dl.T @ h          scale_dW = scale_dl.T @ |h|          flush_dW = flush_dl.T @ |h| + F32_TINY
    err = max over entries with scale > 0 of  max(|got - want| - out_rounding |want| - flush, 0) / scale

and `got` must be exactly 0 wherever scale == 0 (d hidden of rows without a gradient; NaN counts as non-zero).
`out_rounding` is 2^-8 for a result delivered in bf16 and 0 for fp32.  No entry is left out for any other reason.
`flush_dl` is grad_checks' allowance for a probability or a stored value below the smallest normal number, plus two such
values for the two bf16 planes d logits is stored in (bf16 has fp32's exponent range: a low plane below F32_TINY is 0).
With `base` (d W accumulated into a buffer that held `base`), `got - base` is compared and one fp32 rounding (2^-24) of
`|base| + |want|` joins the allowance.

Bounds.  bound = 4 x HEAD_REF[family][product] + HEAD_FORMAT[product]:

* HEAD_REF: the same metric for the reference's own fp32 arithmetic - torch CPU fp32 autograd through
  `h.float() @ W.float().T` and the softmax of reference rl/__init__.py:207-233 (`grad_checks.reference_fp32(hidden=,
  weight=)`) - the largest value over the cases of the family, measured on the CPU, rounded up to two digits.  4 x for a
  different summation order and 1-2 ulp of the hardware exp2, the margin grad_checks uses.
* HEAD_FORMAT: what the operand format of DESIGN.md section 2 costs BY CONSTRUCTION; a worst case, so it gets no factor.
  Round-to-nearest bf16 keeps 8 significant bits: |bf16(x) - x| <= 2^-8 |x| (grad_checks.BF16_ROUNDING).  A value stored as
  hi = bf16(x), lo = bf16(x - hi) therefore has |x - hi| <= 2^-8 |x| and |x - hi - lo| <= 2^-8 |x - hi| <= 2^-16 |x|.
    d W = (dl_hi + dl_lo)^T h, h exact:  |error| <= 2^-16 sum |dl| |h| <= 2^-16 scale_dW          -> 2^-16 = 1.53e-5
    d hidden, bf16 weight = (dl_hi + dl_lo) W, W exact: the same                                  -> 2^-16
    d hidden, fp32 weight = dl_hi W_hi + dl_lo W_hi + dl_hi W_lo.  With dl = dl_hi + dl_lo + e_d, W = W_hi + W_lo + e_w:
        dl W - (the three products) = dl_lo W_lo + e_d W + (dl_hi + dl_lo) e_w,  |dl_lo| <= 2^-8 |dl| (1 + 2^-8),
        |W_lo| <= 2^-8 |W| (1 + 2^-8), |e_d| <= 2^-16 |dl|, |e_w| <= 2^-16 |W|                   -> 3 x 2^-16 (1 + 2^-8) = 4.6e-5
  (sum |dl| |W| <= scale_dH because |want_dl| <= scale_dl entry by entry.)
  `hidden_grad_terms` = 2 drops W_lo from every product: + 2^-8 (the whole rounding of W to bf16); = 1 drops dl_lo as
  well: + 2 x 2^-8.  2^-9 is the MEAN relative rounding of bf16, not its bound: a row whose label term dominates d hidden
  and whose operands sit just above a power of two sees nearly the full 2^-8 of each - the CPU emulation reaches 3.7e-3 =
  0.95 x 2^-8 with one plane dropped and 6.6e-3 = 1.7 x 2^-8 with two (200 .. 900 rows x 128 .. 512 columns).
  `emulate_planes` below restates the three products with nothing from the package (fp64 products of bf16-rounded
  operands); the host test confirms that it stays within HEAD_FORMAT on every family and re-measures HEAD_REF.

Every bound of the default path stays below grad_checks.MUTANT_FLOOR (5e-4), asserted below.  No bound comes from a kernel;
the kernels' measured values are in DESIGN.md section 7 next to the reference's.
"""

from __future__ import annotations

import dataclasses

import numpy as np
import torch

import grad_checks as gc

F32_ROUNDING = 2.0 ** -24

HEAD_FORMAT = {
    "d_weight": 2.0 ** -16,
    "d_hidden_bf16w": 2.0 ** -16,
    "d_hidden_f32w": 3.0 * 2.0 ** -16 * (1.0 + 2.0 ** -8),
}
# what `hidden_grad_terms` = 2 / 1 add to the d hidden allowance of an fp32 weight (a bf16 weight has no low plane: terms = 2
# is its default), and the least the dropped planes must cost - so that the default cannot silently become one of them
TERMS_EXTRA = {3: 0.0, 2: 2.0 ** -8, 1: 2.0 * 2.0 ** -8}

# family -> product -> largest value of the metric for the reference's fp32 arithmetic over the family's cases (CPU)
HEAD_REF = {
    "randn": {"d_hidden": 4.3e-6, "d_weight": 6.7e-6},      # the suite's recipe: W = randn * 2 / sqrt(H), bf16 randn hidden
    "edges": {"d_hidden": 5.0e-6, "d_weight": 6.0e-6},      # randn + label / maximum (+10) / tied maxima on the tile edges
    "trained": {"d_hidden": 3.0e-5, "d_weight": 8.5e-5},    # p(label) up to ~1, flat row and stretches, offset (bf16), T = 0.3 / 0.7 / 2
    "hidden_x8": {"d_hidden": 1.7e-5, "d_weight": 3.6e-5},  # hidden states x 8 (logits of standard deviation 16), bf16 weight
}
# largest absolute error (nats) of new_logprobs / entropy / logsumexp of the reference's fp32 head against fp64
HEAD_FWD_REF = {"randn": 1.0e-5, "edges": 9.3e-6, "trained": 6.6e-5, "hidden_x8": 3.1e-5}
HEAD_FWD_BOUND = {k: 4.0 * v for k, v in HEAD_FWD_REF.items()}


def format_key(product: str, weight_dtype) -> str:
    if product == "d_weight":
        return "d_weight"
    return "d_hidden_bf16w" if weight_dtype == torch.bfloat16 else "d_hidden_f32w"


def head_bound(family: str, product: str, weight_dtype=torch.float32, terms: int = 3) -> float:
    """4 x reference + format term (+ the dropped planes of `hidden_grad_terms` < 3, d hidden of an fp32 weight only)."""
    extra = TERMS_EXTRA[terms] if (product == "d_hidden" and weight_dtype != torch.bfloat16) else 0.0
    return 4.0 * HEAD_REF[family][product] + HEAD_FORMAT[format_key(product, weight_dtype)] + extra


for _f in HEAD_REF:
    for _p in ("d_hidden", "d_weight"):
        for _w in (torch.float32, torch.bfloat16):
            assert head_bound(_f, _p, _w) < gc.MUTANT_FLOOR, (_f, _p, _w)


# ---- where the kernels cut their work ------------------------------------------------------------------------------------
TILE_SHAPES = {"256x256": (256, 256), "256": (256, 128), "128": (128, 128)}  # PRL_LMHEAD_TILE -> (BM vocabulary, BN tokens)
GEMM_TILE = 256   # d hidden / d W product tiles (CfgTriple, CfgDual): 256 x 256
BK32 = 32         # contraction step of the d hidden cores


def ksplit_boundaries(vocab: int, ksplit: int) -> list[int]:
    """First vocabulary index of every split-K slice but the first (d hidden contracts over the vocabulary in steps of 32;
    `ksplit` slices of ceil(steps / ksplit) steps, empty slices dropped; a request above steps / 2 is ignored)."""
    steps = vocab // BK32
    if ksplit < 2 or ksplit > 8 or ksplit > steps // 2:
        return []
    ksteps = -(-steps // ksplit)
    n = -(-steps // ksteps)
    return [i * ksteps * BK32 for i in range(1, n)]


def nsplit_boundaries(vocab: int, bm: int, nsplit: int) -> list[int]:
    """First vocabulary index of every vocabulary range but the first: the d logits (and forward) workgroups of one token
    tile share the ceil(vocab / bm) vocabulary tiles as ranges [vt * s / n, vt * (s + 1) / n)."""
    vt = -(-vocab // bm)
    n = max(1, min(nsplit, vt))
    return sorted({(vt * s // n) * bm for s in range(1, n)} - {0})


def edge_positions(vocab: int, rows: int, bm: int, bn: int, chunk_rows: int | None = None, ksplit=(), nsplit=()) -> dict:
    """Where a wrong index shows: `vocab`: vocabulary rows 0, BM - 1, BM, the last row of the last full tile, the first and
    last row of a partial last tile, V - 1, and both sides of every split-K / vocabulary-range boundary; `token`: logits rows
    0, BN - 1, BN, the last row, and both sides of every chunk boundary.  Positions outside the problem are dropped."""
    v = {0, bm - 1, bm, vocab - 1}
    full = (vocab // bm) * bm
    v |= {full - 1, full}  # full == vocab (no partial tile) is dropped below
    for ks in ksplit:
        for b in ksplit_boundaries(vocab, ks):
            v |= {b - 1, b}
    for ns in nsplit:
        for b in nsplit_boundaries(vocab, bm, ns):
            v |= {b - 1, b}
    t = {0, bn - 1, bn, rows - 1}
    if chunk_rows:
        for b in range(chunk_rows, rows, chunk_rows):
            t |= {b - 1, b}
    return {"vocab": sorted(x for x in v if 0 <= x < vocab), "token": sorted(x for x in t if 0 <= x < rows)}


def locate(product: str, row: int, col: int, bm: int | None = None, bn: int | None = None, chunk_rows: int | None = None) -> str:
    """The tiles an entry lies in.  d hidden [token row, hidden column]; d W [vocabulary row, hidden column]."""
    if product == "d_hidden":
        c = row // chunk_rows if chunk_rows else 0
        rc = row - c * chunk_rows if chunk_rows else row
        s = f"chunk {c} row {rc} of it, product tile ({rc // GEMM_TILE}, {col // GEMM_TILE})"
        return s + (f", d logits token tile {rc // bn} (row {rc % bn})" if bn else "")
    s = f"product tile ({row // GEMM_TILE}, {col // GEMM_TILE})"
    return s + (f", d logits vocabulary tile {row // bm} (row {row % bm})" if bm else "")


# ---- witness ---------------------------------------------------------------------------------------------------------------
def _dev_t(a, device, dtype=None) -> torch.Tensor:
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    return t.detach().to(device=device, dtype=dtype) if dtype is not None else t.detach().to(device)


def logits64(hidden, weight, vocab_block: int = 16384) -> torch.Tensor:
    """h.double() @ W.double().T on the operands' device, the weight converted block by block."""
    h = hidden.detach().double()
    return torch.cat([h @ weight[a:a + vocab_block].detach().double().t() for a in range(0, weight.shape[0], vocab_block)], dim=1)


def dlogits_terms(hidden, weight, ids, g_nlp, g_ent, temperature: float, row_block: int = 32):
    """(want, scale, flush, logits64), fp64 [R, V] torch tensors on the device of `hidden`: grad_checks' witness of d logits
    for the exact logits of the head, with the plane flush added."""
    dev = hidden.device
    x = logits64(hidden, weight)
    ids_t, g, gh = _dev_t(ids, dev, torch.int64), _dev_t(g_nlp, dev, torch.float64), _dev_t(g_ent, dev, torch.float64)
    want, scale, flush = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
    for a in range(0, x.shape[0], row_block):
        b = slice(a, min(a + row_block, x.shape[0]))
        want[b], scale[b], f = gc._witness_block(x[b], ids_t[b], g[b], gh[b], temperature)
        flush[b] = f + 2.0 * gc.F32_TINY
    return want, scale, flush, x


@dataclasses.dataclass
class HeadCheck:
    product: str        # "d_hidden" or "d_weight"
    err: float          # max over entries with scale > 0 of the excess error / scale
    row: int            # token row (d hidden) or vocabulary row (d W)
    col: int            # hidden column
    where: str          # chunk and tiles of the worst entry
    got: float
    want: float
    scale: float
    stray: int          # non-zero entries where scale == 0 (must be 0)
    stray_at: tuple | None

    def __str__(self):
        s = (f"per-entry {self.product} error {self.err:.3e} at row {self.row} col {self.col} ({self.where}): "
             f"got {self.got:.9e} want {self.want:.9e} scale {self.scale:.3e}")
        if self.stray:
            s += f"; {self.stray} non-zero entries where the gradient is exactly 0, first at {self.stray_at}"
        return s

    def ok(self, bound: float) -> bool:
        return self.stray == 0 and self.err <= bound  # NaN fails


class _Worst:
    def __init__(self):
        self.err, self.at, self.vals, self.stray, self.stray_at = -1.0, (0, 0), (0.0, 0.0, 0.0), 0, None

    def update(self, got, want, scale, flush, out_rounding, row0, base=None):
        got = got.double()
        allow = out_rounding * want.abs() + flush
        if base is not None:
            base = base.double()
            got = got - base
            allow = allow + F32_ROUNDING * (base.abs() + want.abs())
        live = scale > 0
        bad = ~live & (got != 0)  # NaN != 0 is true
        n_bad = int(bad.sum())
        if n_bad:
            if self.stray_at is None:
                r, c = bad.nonzero()[0].tolist()
                self.stray_at = (row0 + r, c)
            self.stray += n_bad
        e = ((got - want).abs() - allow).clamp_min(0.0) / torch.where(live, scale, torch.ones_like(scale))
        e = torch.where(live, e, torch.zeros_like(e))
        e = torch.where(torch.isnan(got) & live, torch.full_like(e, float("inf")), e)
        m = float(e.max())
        if m > self.err:
            k = int(e.argmax())
            r, c = divmod(k, e.shape[1])
            self.err, self.at = m, (row0 + r, c)
            self.vals = (float(got[r, c]), float(want[r, c]), float(scale[r, c]))

    def result(self, product, **layout) -> HeadCheck:
        return HeadCheck(product, self.err, self.at[0], self.at[1], locate(product, *self.at, **layout), *self.vals, self.stray, self.stray_at)


def head_errors(got_dh, got_dw, hidden, weight, ids, g_nlp, g_ent, temperature: float, *, dh_rounding: float = 0.0,
                dw_rounding: float = 0.0, dw_base=None, terms=None, bm=None, bn=None, chunk_rows=None, vocab_block: int = 8192):
    """The metric of the module docstring for d hidden [R, H] and d W [V, H] (either may be None) -> (HeadCheck | None,
    HeadCheck | None).  `hidden` [R, H], `weight` [V, H] as stored, `ids` / `g_nlp` / `g_ent` [R] per logits ROW
    (`grad_checks.token_rows`).  Runs on the device of `hidden` (fp64, the weight a block of vocabulary rows at a time).
    `terms`: the (want, scale, flush, logits64) of `dlogits_terms` for the same inputs, shared between variants.
    `dw_base`: what the d W buffer held before an accumulating backward.  `bm`, `bn`, `chunk_rows`: for the message."""
    dev = hidden.device
    want, scale, flush, _ = terms if terms is not None else dlogits_terms(hidden, weight, ids, g_nlp, g_ent, temperature)
    R, V = want.shape
    H = hidden.shape[1]
    h64 = hidden.detach().double()
    habs = h64.abs()
    w_dh = torch.zeros((R, H), dtype=torch.float64, device=dev)
    s_dh, f_dh = torch.zeros_like(w_dh), torch.full_like(w_dh, gc.F32_TINY)
    dw = _Worst()
    for a in range(0, V, vocab_block):
        b = slice(a, min(a + vocab_block, V))
        if got_dh is not None:
            w64 = weight[b].detach().double()
            w_dh += want[:, b] @ w64
            s_dh += scale[:, b] @ w64.abs()
            f_dh += flush[:, b] @ w64.abs()
        if got_dw is not None:
            dw.update(_dev_t(got_dw[b], dev), want[:, b].t() @ h64, scale[:, b].t() @ habs, flush[:, b].t() @ habs + gc.F32_TINY,
                      dw_rounding, a, None if dw_base is None else _dev_t(dw_base[b], dev))
    res_h = None
    if got_dh is not None:
        dh = _Worst()
        dh.update(_dev_t(got_dh, dev), w_dh, s_dh, f_dh, dh_rounding, 0)
        res_h = dh.result("d_hidden", bn=bn, chunk_rows=chunk_rows)
    return res_h, (dw.result("d_weight", bm=bm) if got_dw is not None else None)


def products64(dl, hidden, weight, vocab_block: int = 8192):
    """fp64 (dl @ W, dl^T @ h) of a candidate d logits [R, V] (torch fp64) - what the host test feeds its mutants through."""
    h64 = hidden.detach().double()
    dh = torch.zeros((dl.shape[0], hidden.shape[1]), dtype=torch.float64)
    dw = torch.empty((weight.shape[0], hidden.shape[1]), dtype=torch.float64)
    for a in range(0, weight.shape[0], vocab_block):
        b = slice(a, min(a + vocab_block, weight.shape[0]))
        dh += dl[:, b] @ weight[b].detach().double()
        dw[b] = dl[:, b].t() @ h64
    return dh, dw


# ---- the operand format, restated without the package ------------------------------------------------------------------------
def _bf16(x: torch.Tensor) -> torch.Tensor:
    return x.float().to(torch.bfloat16).double()


def planes(x: torch.Tensor):
    """hi = bf16(x), lo = bf16(x - hi) of the fp32 value x, both as fp64."""
    x = x.float().double()
    hi = _bf16(x)
    return hi, _bf16(x - hi)


def emulate_planes(dl, hidden, weight, hidden_grad_terms: int = 3):
    """(d hidden, d W) fp64 as the operand format of DESIGN.md section 2 forms them from exact d logits `dl` (torch fp64,
    rounded to fp32 first as a kernel holds it): d W = (dl_hi + dl_lo)^T h; d hidden = dl_hi W_hi + dl_lo W_hi + dl_hi W_lo
    for an fp32 weight (`hidden_grad_terms` 2: (dl_hi + dl_lo) W_hi, 1: dl_hi W_hi), (dl_hi + dl_lo) W for a bf16 one.
    Products and sums in fp64: only the format's own loss is left."""
    dl_hi, dl_lo = planes(dl)
    h64 = hidden.detach().double()
    dw = (dl_hi + dl_lo).t() @ h64
    if weight.dtype == torch.bfloat16:
        return (dl_hi + dl_lo) @ weight.double(), dw
    w_hi, w_lo = planes(weight)
    if hidden_grad_terms == 1:
        return dl_hi @ w_hi, dw
    if hidden_grad_terms == 2:
        return (dl_hi + dl_lo) @ w_hi, dw
    return dl_hi @ w_hi + dl_lo @ w_hi + dl_hi @ w_lo, dw
