"""Per-entry checks of the sequence-parallel packed attention (plain torch; no kernel runs here).  The metric, the fp64 witness
and the flash arithmetic are those of tests/attention_checks.py; this file adds the slice form.

A packed row of N tokens is cut into P contiguous slices of L = N / P tokens.  Rank r keeps the queries of `[r L, (r + 1) L)` and
attends them to the keys of the whole row: key j is visible to local query i iff `seq_start[r L + i] <= j <= r L + i`.  out, lse and
dq of a slice are final; dk and dv of a key are sums over the queries of EVERY rank, so each rank produces an fp32 partial over the
whole row and the partials are added in rank order and rounded to bf16 once.

`sp_compose` is that composition in the flash arithmetic of `attention_checks.flash_reference` (fp32 scores, key tiles on the
global 64-grid, the unnormalised P rounded to bf16, fp32 accumulation), with one switch per seeded mistake.

Bounds.  bound = 4 x ATTN_SP_FLASH[case][output].  ATTN_SP_FLASH is the metric of the UNSLICED `flash_reference` on the whole row
against the fp64 witness: the largest value over the heads and head sizes of the case, measured on the CPU
(tests/test_attention_sp_checks_host.py re-measures it), under `attention_checks.table_figure` (plus a tenth, two digits, lse
floored at 2^-24).  No figure comes from a kernel, and none from the sliced arithmetic: slicing changes only the order in which
the terms of dk / dv are added (per rank, then over the ranks) and, at an offset that is no multiple of 64, which queries share a
block - different but equally valid summation orders, which is what the project's standing 4 x margin is for.
"""

from __future__ import annotations

import dataclasses

import torch

import attention_checks as ac
from attention_checks import OUTPUTS, bf16_exact, measure, rounding, table_figure, visible  # noqa: F401

HEADS = ((4, 2), (7, 1))
HEAD_SIZES = (64, 128)
TILE = 64

# case -> output -> the metric of the unsliced `flash_reference` on the whole row, largest over HEADS x HEAD_SIZES (CPU, torch 2.10),
# under table_figure
ATTN_SP_FLASH = {
    "sp_aligned": {"out": 4.3e-3, "lse": 1.5e-7, "dq": 1.1e-3, "dk": 1.1e-3, "dv": 5.3e-3},
    "sp_unaligned": {"out": 4.7e-3, "lse": 1.2e-7, "dq": 1.4e-3, "dk": 1.1e-3, "dv": 4.9e-3},
    "sp_four": {"out": 5.1e-3, "lse": 1.3e-7, "dq": 1.5e-3, "dk": 1.2e-3, "dv": 5.7e-3},
    "sp_long": {"out": 5.1e-3, "lse": 1.5e-7, "dq": 1.6e-3, "dk": 1.6e-3, "dv": 5.7e-3},
}


def bound(case: str, output: str) -> float:
    return 4.0 * ATTN_SP_FLASH[case][output]


@dataclasses.dataclass(frozen=True)
class SpCase:
    name: str
    lengths: tuple      # the sequences of the whole row, in order
    p: int              # slices
    score: float = 4.0
    ramp: bool = False

    @property
    def n(self) -> int:
        return sum(self.lengths)

    @property
    def slice_len(self) -> int:
        assert self.n % self.p == 0
        return self.n // self.p

    @property
    def base(self) -> ac.Case:
        return ac.Case(self.name, self.lengths, score=self.score, ramp=self.ramp)


CASES = (
    # the cut is on a block edge; the second sequence crosses it
    SpCase("sp_aligned", (100, 156), 2),
    # L = 129: the offset is neither a block nor an 8-element multiple; rank 1's sweep starts inside rank 0's keys
    SpCase("sp_unaligned", (40, 218), 2),
    # L = 96: a sequence starts exactly on a cut (96), a length-1 sequence, one sequence (97 .. 295) spans three ranks
    SpCase("sp_four", (96, 1, 199, 88), 4),
    # one sequence, scores up to +-60, the maximum moving per key block; the last rank's dk / dv partials reach back to rank 0
    SpCase("sp_long", (384,), 4, score=20.0, ramp=True),
)


def problem(case: SpCase, hq: int, hkv: int, d: int):
    """(q, k, v, g, scale, seq_start, seq_end) of the whole row."""
    q, k, v, g, scale = ac.inputs(case.base, hq, hkv, d)
    ss, se = ac.table_of(case.lengths)
    return q, k, v, g, scale, ss, se


def fold(parts: list, skip: int | None = None, parts_bf16: bool = False) -> torch.Tensor:
    """rne(parts[0] + parts[1] + ...): fp32, rank order, one rounding.  The two mistakes: rank `skip` left out; every partial rounded
    to bf16 before the sum."""
    acc = None
    for r, part in enumerate(parts):
        if r == skip:
            continue
        part = bf16_exact(part) if parts_bf16 else part.float()
        acc = part.clone() if acc is None else acc + part
    return bf16_exact(acc)


def slice_flash(q_loc, k, v, g_loc, seq_start, scale: float, q_off: int, tile: int = TILE, *, drop_offset: bool = False,
                restart_at_cut: bool = False) -> dict:
    """The flash arithmetic of `attention_checks.flash_reference` for the `nq` local queries at `q_off` against the whole row:
    out, lse, dq as delivered, `dk_part` / `dv_part` in fp32 over the whole row (zeros where no local query sees the key).
        drop_offset     the causal compare takes the LOCAL query index (j <= i instead of j <= q_off + i)
        restart_at_cut  seq_start of the local queries clamped to q_off: a sequence that crosses the cut starts again there"""
    q_loc, k, v, g_loc = (t.detach().float().cpu() for t in (q_loc, k, v, g_loc))
    nq, hq, d = q_loc.shape
    nk, hkv = k.shape[0], k.shape[1]
    grp = hq // hkv
    qh, gh = q_loc.transpose(0, 1), g_loc.transpose(0, 1)  # [Hq, nq, D]
    kh, vh = (t.repeat_interleave(grp, dim=1).transpose(0, 1) for t in (k, v))  # [Hq, nk, D]
    first = seq_start.long().cpu()[q_off:q_off + nq]
    if restart_at_cut:
        first = first.clamp(min=q_off)
    i = torch.arange(nq).view(nq, 1) + (0 if drop_offset else q_off)
    j = torch.arange(nk).view(1, nk)
    vis = (j <= i) & (j >= first.view(nq, 1))  # [nq, nk]

    out = torch.zeros(hq, nq, d)
    lse = torch.zeros(hq, nq)
    for l0 in range(0, nq, tile):
        rows = slice(l0, min(l0 + tile, nq))
        width = rows.stop - l0
        m = torch.full((hq, width), float("-inf"))
        l = torch.zeros(hq, width)
        o = torch.zeros(hq, width, d)
        for k0 in range(int(first[l0]) // tile * tile, q_off + rows.stop, tile):  # key tiles on the global grid, up to the diagonal
            cols = slice(k0, min(k0 + tile, nk))
            y = ((qh[:, rows] @ kh[:, cols].transpose(1, 2)) * scale).masked_fill(~vis[rows, cols], float("-inf"))
            mn = torch.maximum(m, y.amax(-1))
            at = torch.where(torch.isinf(mn), torch.zeros_like(mn), mn)
            alpha = torch.exp(m - at)
            p = torch.exp(y - at.unsqueeze(-1))
            l = l * alpha + p.sum(-1)
            o = o * alpha.unsqueeze(-1) + bf16_exact(p) @ vh[:, cols]
            m = mn
        out[:, rows] = bf16_exact(o / l.unsqueeze(-1))
        lse[:, rows] = m + torch.log(l)

    p = torch.where(vis, torch.exp((qh @ kh.transpose(1, 2)) * scale - lse.unsqueeze(-1)), torch.zeros(()))
    dp = gh @ vh.transpose(1, 2)
    delta = (gh * out).sum(-1, keepdim=True)
    ds = bf16_exact(p * (dp - delta))
    pb = bf16_exact(p)
    heads = lambda t: t.view(hkv, grp, nk, d).sum(1).transpose(0, 1)  # noqa: E731  [Hq, nk, D] -> [nk, Hkv, D]
    return {
        "out": out.transpose(0, 1),
        "lse": lse,
        "dq": bf16_exact(scale * (ds @ kh)).transpose(0, 1),
        "dk_part": scale * heads(ds.transpose(1, 2) @ qh),
        "dv_part": heads(pb.transpose(1, 2) @ gh),
    }


MISTAKES = {  # name -> the switches of sp_compose it sets
    "offset_dropped": {"drop_offset": True},
    "restart_at_cut": {"restart_at_cut": True},
    "rank_left_out": {"skip_last_rank": True},
    "parts_bf16": {"parts_bf16": True},
}


def sp_compose(q, k, v, g, seq_start, scale: float, p: int, *, drop_offset: bool = False, restart_at_cut: bool = False,
               skip_last_rank: bool = False, parts_bf16: bool = False) -> dict:
    """The five results of the whole row from P serial slices: out, lse, dq concatenated, dk / dv folded in rank order."""
    n = q.shape[0]
    assert n % p == 0
    length = n // p
    runs = [slice_flash(q[r * length:(r + 1) * length], k, v, g[r * length:(r + 1) * length], seq_start, scale, r * length,
                        drop_offset=drop_offset, restart_at_cut=restart_at_cut) for r in range(p)]
    skip = p - 1 if skip_last_rank else None
    return {
        "out": torch.cat([r["out"] for r in runs], dim=0),
        "lse": torch.cat([r["lse"] for r in runs], dim=1),
        "dq": torch.cat([r["dq"] for r in runs], dim=0),
        "dk": fold([r["dk_part"] for r in runs], skip, parts_bf16),
        "dv": fold([r["dv_part"] for r in runs], skip, parts_bf16),
    }


def check_outputs(case: str, label: str, got: dict, wit: dict, verbose: bool = True) -> dict:
    """Every output of `got` against the witness under bound(case, output); prints each figure before it asserts."""
    return ac.check_outputs(case, label, got, wit, limits={name: bound(case, name) for name in got}, verbose=verbose)
