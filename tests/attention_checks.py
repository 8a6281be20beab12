"""Per-entry checks of the packed varlen attention - out, lse, dq, dk, dv (plain torch; no kernel runs here).  The scheme of
tests/body_checks.py: an fp64 witness from the bf16 input values, the size of each entry's own terms as its scale, and

    err = max over entries with scale > 0 of  max(|got - want| - rounding |want|, 0) / scale

`got` must be exactly 0 wherever scale == 0 (NaN counts as non-zero).  `rounding` is 2^-9 for a result delivered in bf16 (half
a unit in the last of 8 significant bits) and 0 for the fp32 `lse`.

For q [N, Hq, D], k, v [N, Hkv, D], upstream dO [N, Hq, D], a segment table `seq_start` (key j visible to query i iff
seq_start[i] <= j <= i) and query head h reading KV head h // (Hq / Hkv):
    s = scale q k^T       lse = ln sum_j exp(s)      p = exp(s - lse)             (over the visible j)
    out = p v                                   scale sum_j |p v|
    lse                                         scale 1 + sum_j p sum_d |scale q k|   (the unit of a logarithm + the terms of the scores it weighs)
    dp = dO v^T    delta = sum_d dO out    ds = p (dp - delta)      |ds|' = p (|dO| |v|^T + sum_d |dO out|): dp and delta cancel where
                                                                      one key holds all the weight, their terms do not
    dq = scale ds k                             scale sum_j |ds|' |k| scale
    dk = scale sum_{h in group} ds^T q          scale sum |ds|' |q| scale
    dv = sum_{h in group} p^T dO                scale sum |p dO|

Bounds.  bound = 4 x ATTN_FLASH[case][output].  ATTN_FLASH is the same metric for `flash_reference`: the published
flash-attention arithmetic in plain torch on the CPU - fp32 scores from the bf16 inputs, 64-key tiles, online softmax, the
unnormalised P rounded to bf16, fp32 accumulation, results rounded to bf16; the backward takes P from the fp32 `lse`, rounds P and
dS to bf16 and forms delta from the bf16 `out`.  That is the arithmetic of the reference project's real path (flash-attn varlen)
and the error model of the kernels: what is left is the rounding of P, of dS and of the result.  Each entry is the largest value
over the heads and head sizes of the case, measured on the CPU (tests/test_attention_checks_host.py re-measures it), plus a tenth
(a maximum over entries moves a little with the CPU's blocking and thread count), rounded up to two digits; for the fp32 `lse`
the figure is floored at 2^-24 (it sits at the fp32 rounding of a logarithm and moves with the CPU's libm).  4 x is the project's
standing margin for a different but equally valid summation order.

ATTN_REF is the same figure for the other reference op sequence - transformers' `eager_attention_forward` formula (repeat_kv,
q k^T * scaling + additive block-diagonal mask, softmax in fp32 cast back to bf16, @ v) evaluated on the CPU in bf16, backward by
autograd (`reference`).  It rounds the SCORES to bf16, which no flash kernel does, so 4 x ATTN_REF lies 10 - 100 times above
4 x ATTN_FLASH: it is kept as a ceiling (the host suite asserts ATTN_FLASH <= ATTN_REF entry by entry) and to show which seeded
mistakes of `flash_reference` those looser bounds let through.  No bound comes from a kernel; the kernels' values are in
DESIGN.md section 3c.
"""

from __future__ import annotations

import dataclasses
import math

import torch

from body_checks import measure  # the metric itself is shared  # noqa: F401

BF16_ROUNDING = 2.0 ** -9
OUTPUTS = ("out", "lse", "dq", "dk", "dv")

# case -> output -> largest value of the metric for the reference's bf16 op sequence over the heads and head sizes of the case
# (CPU, torch 2.10).  The reference rounds the SCORES to bf16: half a unit in the last place of a score of 16 is 0.06 in the
# exponent, of a score of 60 (case "long") 0.25 - that, not the rounding of p, is what these figures are.
ATTN_REF = {
    "edges": {"out": 7.2e-2, "lse": 2.6e-3, "dq": 9.0e-3, "dk": 9.1e-3, "dv": 7.7e-2},
    "ones": {"out": 6.7e-2, "lse": 2.8e-3, "dq": 9.8e-3, "dk": 8.2e-3, "dv": 5.4e-2},
    "long": {"out": 4.5e-1, "lse": 2.8e-3, "dq": 7.2e-2, "dk": 4.4e-2, "dv": 3.1e-1},
    "b2": {"out": 1.4e-1, "lse": 2.7e-3, "dq": 1.1e-2, "dk": 8.6e-3, "dv": 6.7e-2},
    "padded": {"out": 5.5e-2, "lse": 2.2e-3, "dq": 8.1e-3, "dk": 7.4e-3, "dv": 4.6e-2},
}


LSE_FLOOR = 2.0 ** -24  # half a unit in the last place of an fp32 value in [1, 2): the floor optim_checks.py uses for an fp32 reference

# case -> output -> largest value of the metric for `flash_reference` (no mistake switched on) over the heads and head sizes of the
# case (CPU, torch 2.10), plus a tenth, rounded up to two digits; lse floored at LSE_FLOOR.  What is left after fp32 scores: the
# rounding of P and dS to bf16 and of the result.
ATTN_FLASH = {
    "edges": {"out": 5.1e-3, "lse": 1.2e-7, "dq": 9.8e-4, "dk": 1.4e-3, "dv": 5.7e-3},
    "ones": {"out": 5.1e-3, "lse": 1.4e-7, "dq": 9.6e-4, "dk": 1.5e-3, "dv": 5.6e-3},
    "long": {"out": 5.2e-3, "lse": 1.1e-7, "dq": 1.1e-3, "dk": 1.3e-3, "dv": 6.0e-3},
    "b2": {"out": 4.8e-3, "lse": 1.2e-7, "dq": 1.4e-3, "dk": 1.3e-3, "dv": 5.5e-3},
    "padded": {"out": 4.6e-3, "lse": 9.6e-8, "dq": 8.9e-4, "dk": 7.8e-4, "dv": 5.1e-3},
    "long_mild": {"out": 5.1e-3, "lse": 1.4e-7, "dq": 8.2e-4, "dk": 1.3e-3, "dv": 5.3e-3},
    "mid": {"out": 4.4e-3, "lse": 1.3e-7, "dq": 1.2e-3, "dk": 1.6e-3, "dv": 5.3e-3},
    "mid_ramp": {"out": 5.0e-3, "lse": 1.3e-7, "dq": 1.4e-3, "dk": 1.9e-3, "dv": 6.2e-3},
    "sink": {"out": 2.9e-3, "lse": 8.5e-8, "dq": 1.7e-3, "dk": 1.6e-3, "dv": 5.5e-3},
    "flat": {"out": 2.2e-3, "lse": 2.5e-7, "dq": 6.6e-4, "dk": 0.0, "dv": 3.2e-3},  # dk: q = 0, every term of dk is 0 and so is dk
    "scaled": {"out": 4.6e-3, "lse": 1.4e-7, "dq": 1.8e-3, "dk": 1.6e-3, "dv": 5.1e-3},
    "scale_one": {"out": 5.6e-3, "lse": 1.2e-7, "dq": 1.4e-3, "dk": 1.3e-3, "dv": 5.9e-3},
}


def table_figure(measured: float, output: str) -> float:
    """The rule of both tables: the measured maximum (for lse at least LSE_FLOOR) plus a tenth, rounded up to two digits."""
    x = 1.1 * max(measured, LSE_FLOOR if output == "lse" else 0.0)
    if x == 0.0:
        return 0.0
    unit = 10.0 ** (math.floor(math.log10(x)) - 1)
    return math.ceil(x / unit - 1e-9) * unit


def bound(case: str, output: str) -> float:
    return 4.0 * ATTN_FLASH[case][output]


def old_bound(case: str, output: str) -> float:
    """The bound before ATTN_FLASH set it, for the five cases ATTN_REF has: what the seeded mistakes are also held to."""
    return 4.0 * ATTN_REF[case][output]


def rounding(output: str) -> float:
    return 0.0 if output == "lse" else BF16_ROUNDING


def bf16_exact(t: torch.Tensor) -> torch.Tensor:
    return t.float().to(torch.bfloat16).float()


# ---- the case family -----------------------------------------------------------------------------------------------------------
HEADS = ((1, 1), (4, 2), (7, 1))
HEAD_SIZES = (64, 128)


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    lengths: tuple            # the sequences of the flat batch, in order
    score: float = 4.0        # standard deviation of scale * q . k
    ramp: bool = False        # keys grow block by block: the running maximum of a row moves in every key block
    scale: float | None = None  # the softmax scale handed to the op (None: d ** -0.5); q is sized so that `score` holds under it
    sink: float = 0.0         # not 0: the first key of every sequence is (sink, 0, 0, ...) and every query's component 0 is 1.5 sqrt(d)

    @property
    def n(self) -> int:
        return sum(self.lengths)


def cases(bq: int, bk: int) -> list[Case]:
    """Segment layouts at the kernels' edges, N up to 4 max(BQ, BK) + 1."""
    b = max(bq, bk)
    n = 3 * b + 1
    edges = (b - 1, 1, 1, b // 2 + 3, n - (b + 1) - (b // 2 + 3))
    mid = (40, 4 * b + 1 - 40)
    return [
        # boundaries one before, at and one after a block edge, and one in the middle of a block; length-1 sequences in the middle
        Case("edges", edges),
        # sequences of length 1 at the start, in the middle and at the end
        Case("ones", (1, (n - 3) // 2, 1, n - 3 - (n - 3) // 2, 1)),
        # one sequence over more than 3 key blocks, scores up to +-60 and beyond, the largest ones in the last block
        Case("long", (n,), score=20.0, ramp=True),
        # B = 2, unpadded: a boundary on a block edge when T is one
        Case("b2", (b + b // 2, b + b // 2)),
        # a left-padded and a right-padded row of T = 40: every pad token is a sequence of its own
        Case("padded", (1,) * 5 + (35,) + (30,) + (1,) * 10),
        # one sequence over more than 3 key blocks under ordinary scores: the mask-free tiles without the ramp
        Case("long_mild", (n,)),
        # the second sequence starts inside a block and runs past three more block edges: its later query blocks sweep a partly
        # staged first tile, then mask-free tiles, then the diagonal; the key block that holds the boundary sweeps mask-free
        # query tiles of the second sequence only
        Case("mid", mid),
        Case("mid_ramp", mid, score=20.0, ramp=True),
        # the first key of each sequence dominates (+ 24 on its score): the maximum is set in the first tile and never moves, later
        # P are tiny, dP and delta cancel
        Case("sink", mid, sink=16.0),
        # q = 0: every visible key weighs the same, lse = ln(length so far), out = the running mean of v
        Case("flat", edges, score=0.0),
        # a scale that is neither a power of two nor 1 / sqrt(64) or 1 / sqrt(128) (exact in bf16 and fp32), and scale 1
        Case("scaled", edges, scale=0.09375),
        Case("scale_one", (b + b // 2, b + b // 2), scale=1.0),
    ]


def table_of(lengths, device="cpu") -> tuple[torch.Tensor, torch.Tensor]:
    """(seq_start, seq_end) int32 [N] of consecutive sequences of these lengths, in plain Python."""
    start, end, at = [], [], 0
    for length in lengths:
        start += [at] * length
        end += [at + length] * length
        at += length
    return torch.tensor(start, dtype=torch.int32, device=device), torch.tensor(end, dtype=torch.int32, device=device)


def inputs(case: Case, hq: int, hkv: int, d: int, block: int = 64, seed: int | None = None):
    """(q, k, v, dO) fp32 holding bf16-exact values, and the case's scale (1 / sqrt(d) unless the case names one).  scale * q . k
    has standard deviation `case.score`; with `ramp` the keys of block b are multiplied by 2^(b - 2), so a row's largest score
    arrives last; with `sink` the first key of every sequence gets about 1.5 * sink more than the others."""
    gen = torch.Generator().manual_seed(case.n * 1009 + hq * 101 + hkv * 11 + d if seed is None else seed)
    n = case.n
    q = torch.randn(n, hq, d, generator=gen) * case.score
    k = torch.randn(n, hkv, d, generator=gen)
    v = torch.randn(n, hkv, d, generator=gen)
    g = torch.randn(n, hq, d, generator=gen)
    if case.ramp:
        k = k * (2.0 ** (torch.arange(n) // block - 2).clamp(max=0).float()).view(n, 1, 1)
    scale = 1.0 / math.sqrt(d)
    if case.scale is not None:
        q = q * (scale / case.scale)
        scale = case.scale
    if case.sink:
        firsts = torch.tensor([sum(case.lengths[:i]) for i in range(len(case.lengths))])
        k[firsts] = 0.0
        k[firsts, :, 0] = case.sink
        q[:, :, 0] = 1.5 / scale  # scale * q_0 * sink = 1.5 * sink more on the first key's score
    return bf16_exact(q), bf16_exact(k), bf16_exact(v), bf16_exact(g), scale


def visible(seq_start: torch.Tensor) -> torch.Tensor:
    """bool [N, N]: key j visible to query i."""
    n = seq_start.numel()
    i = torch.arange(n).view(n, 1)
    j = torch.arange(n).view(1, n)
    return (j <= i) & (j >= seq_start.long().cpu().view(n, 1))


# ---- witness (fp64) ------------------------------------------------------------------------------------------------------------
def witness(q, k, v, g, seq_start, scale: float) -> dict:
    """output -> (want, scale), fp64, dense over the N x N scores (N is a few hundred here)."""
    q, k, v, g = (t.detach().double().cpu() for t in (q, k, v, g))
    n, hq, d = q.shape
    hkv = k.shape[1]
    grp = hq // hkv
    kk = k.repeat_interleave(grp, dim=1)  # [N, Hq, D]: head h reads KV head h // grp
    vv = v.repeat_interleave(grp, dim=1)
    vis = visible(seq_start).unsqueeze(0)  # [1, N, N]
    qh, kh, vh, gh = (t.transpose(0, 1) for t in (q, kk, vv, g))  # [Hq, N, D]
    s = scale * qh @ kh.transpose(1, 2)
    s_abs = scale * qh.abs() @ kh.abs().transpose(1, 2)
    s = s.masked_fill(~vis, float("-inf"))
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - lse.unsqueeze(-1))
    out = p @ vh
    dp = gh @ vh.transpose(1, 2)
    delta = (gh * out).sum(-1, keepdim=True)
    ds = p * (dp - delta)
    ds_abs = p * (gh.abs() @ vh.abs().transpose(1, 2) + (gh * out).abs().sum(-1, keepdim=True))  # the terms of dp and of delta
    dq = scale * ds @ kh
    dk_h = scale * ds.transpose(1, 2) @ qh
    dv_h = p.transpose(1, 2) @ gh
    fold = lambda t: t.view(hkv, grp, n, d).sum(1).transpose(0, 1)  # noqa: E731  [Hq, N, D] -> [N, Hkv, D]
    tok = lambda t: t.transpose(0, 1)  # noqa: E731
    return {
        "out": (tok(out), tok(p @ vh.abs())),
        "lse": (lse, 1.0 + (p * s_abs).sum(-1)),
        "dq": (tok(dq), tok(scale * ds_abs @ kh.abs())),
        "dk": (fold(dk_h), fold(scale * ds_abs.transpose(1, 2) @ qh.abs())),
        "dv": (fold(dv_h), fold(p.transpose(1, 2) @ gh.abs())),
    }


def naive(q, k, v, g, lengths, scale: float) -> dict:
    """The same five results sequence by sequence, by torch autograd in fp64 on each sequence alone."""
    outs = {name: [] for name in OUTPUTS}
    at = 0
    grp = q.shape[1] // k.shape[1]
    for length in lengths:
        sl = slice(at, at + length)
        qs, ks, vs = (t[sl].detach().double().clone().requires_grad_(True) for t in (q, k, v))
        s = scale * torch.einsum("ihd,jhd->hij", qs, ks.repeat_interleave(grp, dim=1))
        s = s.masked_fill(torch.ones(length, length).triu(1).bool(), float("-inf"))
        o = torch.einsum("hij,jhd->ihd", torch.softmax(s, -1), vs.repeat_interleave(grp, dim=1))
        o.backward(g[sl].double())
        for name, t in (("out", o.detach()), ("lse", torch.logsumexp(s.detach(), -1)), ("dq", qs.grad), ("dk", ks.grad), ("dv", vs.grad)):
            outs[name].append(t)
        at += length
    return {name: torch.cat(ts, dim=1 if name == "lse" else 0) for name, ts in outs.items()}


# ---- the reference op sequence, bf16 on the CPU ----------------------------------------------------------------------------------
def reference(q, k, v, g, seq_start, scale: float) -> dict:
    """transformers' eager_attention_forward, operation by operation, in bf16 with the additive block-diagonal mask."""
    qb, kb, vb = (t.detach().to(torch.bfloat16).clone().requires_grad_(True) for t in (q, k, v))
    grp = q.shape[1] // k.shape[1]
    query, key, value = (t.transpose(0, 1).unsqueeze(0) for t in (qb, kb, vb))  # [1, H, N, D]
    key, value = key.repeat_interleave(grp, dim=1), value.repeat_interleave(grp, dim=1)  # repeat_kv
    mask = torch.zeros(visible(seq_start).shape, dtype=torch.bfloat16).masked_fill(~visible(seq_start), torch.finfo(torch.bfloat16).min)
    attn_weights = torch.matmul(query, key.transpose(2, 3)) * scale
    attn_weights = attn_weights + mask
    lse = torch.logsumexp(attn_weights.detach().float(), dim=-1)[0]
    attn_weights = torch.nn.functional.softmax(attn_weights, dim=-1, dtype=torch.float32).to(query.dtype)
    attn_output = torch.matmul(attn_weights, value).transpose(1, 2).contiguous()[0]  # [N, Hq, D]
    attn_output.backward(g.detach().to(torch.bfloat16))
    return {"out": attn_output.detach(), "lse": lse, "dq": qb.grad, "dk": kb.grad, "dv": vb.grad}


# ---- the flash arithmetic, fp32 / bf16 on the CPU: the kernels' error model, and the seeded mistakes -----------------------------
SCALE_USES = ("fwd_exp", "bwd_exp", "dq", "dk")  # where `scale` enters: the two exponents and the two gradient factors
MISTAKES = {  # name -> the switches of flash_reference it sets (each changes one line there)
    "scores_bf16": {"scores_bf16": True},
    "sum_not_rescaled": {"sum_not_rescaled": True},
    "lse_bf16": {"lse_bf16": True},
    "whole_too_early": {"whole_too_early": True},
    **{f"fixed_scale_{use}": {"fixed_scale": use} for use in SCALE_USES},
}


def flash_reference(q, k, v, g, seq_start, scale: float, tile: int = 64, *, scores_bf16: bool = False, sum_not_rescaled: bool = False,
                    lse_bf16: bool = False, whole_too_early: bool = False, fixed_scale: str | None = None) -> dict:
    """The published flash-attention algorithm (Dao et al.: tiled online softmax forward, backward recomputing P from the saved
    logsumexp) as DESIGN.md section 3c describes this library's form of it, in plain torch: fp32 scores from the bf16 inputs,
    key tiles of `tile`, the unnormalised P rounded to bf16 for P V (the row sum takes the fp32 P), fp32 accumulation, results
    rounded to bf16 once; backward with P = exp(s - lse) from the fp32 lse, delta from the bf16 out, P and dS rounded to bf16,
    the query heads of a KV head summed in fp32.  Visibility is `visible()`.  The keyword switches are the seeded mistakes of
    tests/test_attention_checks_host.py, one line each:
        scores_bf16       the scores rounded to bf16 before every exponential
        sum_not_rescaled  the running sum not multiplied by alpha when the running maximum moves
        lse_bf16          lse rounded to bf16 before the backward reads it (the returned lse stays fp32)
        whole_too_early   the key tile that holds a query's seq_start taken without a mask by every later query block
        fixed_scale       one of SCALE_USES: d ** -0.5 instead of `scale` in that one use"""
    q, k, v, g = (t.detach().float().cpu() for t in (q, k, v, g))
    n, hq, d = q.shape
    hkv = k.shape[1]
    grp = hq // hkv
    qh, gh = q.transpose(0, 1), g.transpose(0, 1)  # [Hq, N, D]
    kh, vh = (t.repeat_interleave(grp, dim=1).transpose(0, 1) for t in (k, v))
    assert fixed_scale is None or fixed_scale in SCALE_USES
    sc = {use: d ** -0.5 if fixed_scale == use else scale for use in SCALE_USES}
    first = seq_start.long().cpu()
    vis = visible(seq_start)
    if whole_too_early:
        blk = torch.arange(n) // tile
        vis = vis | ((blk.view(1, n) == (first // tile).view(n, 1)) & (blk.view(1, n) < blk.view(n, 1)))

    def scores(rows, cols, s):
        y = (qh[:, rows] @ kh[:, cols].transpose(1, 2)) * s
        return bf16_exact(y) if scores_bf16 else y

    out = torch.zeros(hq, n, d)
    lse = torch.zeros(hq, n)
    for q0 in range(0, n, tile):
        rows = slice(q0, min(q0 + tile, n))
        m = torch.full((hq, rows.stop - q0), float("-inf"))
        l = torch.zeros(hq, rows.stop - q0)
        o = torch.zeros(hq, rows.stop - q0, d)
        for k0 in range(int(first[q0]) // tile * tile, rows.stop, tile):  # from the tile that holds the block's first visible key
            cols = slice(k0, min(k0 + tile, n))
            y = scores(rows, cols, sc["fwd_exp"]).masked_fill(~vis[rows, cols], float("-inf"))
            mn = torch.maximum(m, y.amax(-1))
            at = torch.where(torch.isinf(mn), torch.zeros_like(mn), mn)  # a row that has seen no key yet
            alpha = torch.exp(m - at)
            p = torch.exp(y - at.unsqueeze(-1))
            l = (l if sum_not_rescaled else l * alpha) + p.sum(-1)
            o = o * alpha.unsqueeze(-1) + bf16_exact(p) @ vh[:, cols]
            m = mn
        out[:, rows] = bf16_exact(o / l.unsqueeze(-1))
        lse[:, rows] = m + torch.log(l)

    every = slice(0, n)
    saved = bf16_exact(lse) if lse_bf16 else lse
    p = torch.where(vis, torch.exp(scores(every, every, sc["bwd_exp"]) - saved.unsqueeze(-1)), torch.zeros(()))
    dp = gh @ vh.transpose(1, 2)
    delta = (gh * out).sum(-1, keepdim=True)
    ds = bf16_exact(p * (dp - delta))
    pb = bf16_exact(p)
    fold = lambda t: t.view(hkv, grp, n, d).sum(1).transpose(0, 1)  # noqa: E731  [Hq, N, D] -> [N, Hkv, D]
    return {
        "out": out.transpose(0, 1),
        "lse": lse,
        "dq": bf16_exact(sc["dq"] * (ds @ kh)).transpose(0, 1),
        "dk": bf16_exact(sc["dk"] * fold(ds.transpose(1, 2) @ qh)),
        "dv": bf16_exact(fold(pb.transpose(1, 2) @ gh)),
    }


def check_outputs(case: str, label: str, got: dict, wit: dict, limits=None, verbose: bool = True) -> dict:
    """Every output of `got` against the witness under bound(case, output); prints each figure before it asserts."""
    errs, failed = {}, []
    for name, value in got.items():
        want, scale = wit[name]
        res = measure(name, value, want, scale, rounding(name))
        errs[name] = res.err
        limit = bound(case, name) if limits is None else limits[name]
        if verbose:
            print(f"[attention] {label}: {res} (bound {limit:.2e})")
        if not res.ok(limit):
            failed.append(str(res) + f" > bound {limit:.3e}")
    assert not failed, f"{label}: " + "; ".join(failed)
    return errs


# ---- segment tables: the rule in plain Python, and the [B, T] inputs both forms of segments() are run on ---------------------------
def plain_segments(position_ids, attention_mask, batch, t):
    start, end = [0] * (batch * t), [0] * (batch * t)
    for b in range(batch):
        begins = []
        for c in range(t):
            new = c == 0
            if position_ids is not None and c > 0 and position_ids[b][c] != position_ids[b][c - 1] + 1:
                new = True
            if attention_mask is not None and c > 0 and (attention_mask[b][c] == 0 or attention_mask[b][c - 1] == 0):
                new = True
            if new:
                begins.append(c)
        begins.append(t)
        for s, e in zip(begins[:-1], begins[1:]):
            for c in range(s, e):
                start[b * t + c], end[b * t + c] = b * t + s, b * t + e
    return start, end


def segment_cases():
    """name -> (position_ids or None, attention_mask or None, (B, T)) as nested lists."""
    ar = lambda n: list(range(n))  # noqa: E731
    return {
        "packed": ([ar(5) + ar(7)], None, (1, 12)),
        "packed_mask_ones": ([ar(5) + ar(7)], [[1] * 12], (1, 12)),
        "length_one": ([ar(4) + [0] + ar(3) + [0]], None, (1, 9)),
        "sp_filler": ([ar(5) + ar(7) + ar(3)], [[1] * 15], (1, 15)),  # the sequence-parallel filler is one more packed slot
        "left_right_padding": (None, [[0, 0, 0, 1, 1, 1, 1, 1], [1, 1, 1, 1, 1, 1, 0, 0]], (2, 8)),
        "padding_with_positions": ([[0, 0, 0, 0, 1, 2, 3, 4], [0, 1, 2, 3, 4, 5, 0, 0]], [[0, 0, 0, 1, 1, 1, 1, 1], [1, 1, 1, 1, 1, 1, 0, 0]], (2, 8)),
        "b3_packed": ([ar(6), ar(2) + ar(4), ar(3) + ar(3)], None, (3, 6)),
        "nothing": (None, None, (2, 5)),
        "one_token": ([[0]], [[1]], (1, 1)),
    }


def sized_segment_case(t: int):
    """A packed row of T tokens in sequences of 1, 2, 3, ... tokens."""
    pos, length = [], 1
    while len(pos) < t:
        pos += list(range(min(length, t - len(pos))))
        length += 1
    return [pos], None, (1, t)
