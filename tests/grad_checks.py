"""Per-entry, condition-aware check of d loss / d logits (plain torch-CPU / numpy; no kernel runs here).

Why: `helpers.rel_err` is `max|got - want| / max|want|`.  A full-vocabulary row of d logits is one label entry of size ~g
and ~152 000 softmax entries of size g * p_v with p_v ~ 1e-6 .. 1e-4, so a tolerance of 1e-4 of the global maximum is
larger than 99.8 % of the entries: a kernel that zeroes them all, drops one 16-byte vector or scales the whole softmax
body by 1.001 passes.  Here every entry is measured against the size of ITS OWN terms before they cancel.

For a logits row with label `id`, token gradients g = d loss / d new_logprob, gH = d loss / d entropy and temperature T:

    want_v  = (g (1[v = id] - p_v) - gH p_v (ln p_v + H)) / T            (fp64 closed form, the suite's witness)
    scale_v = (|g| (1[v = id] + p_v) + |gH| p_v (|ln p_v| + |H|)) / T     (the same terms, absolute values)
    err     = max_v  max(|got_v - want_v| - out_rounding |want_v| - flush_v, 0) / scale_v      over scale_v > 0

and got_v must be exactly 0 wherever scale_v == 0 (rows without gradient, entries whose p_v is 0 in fp64).
`out_rounding` is the rounding of the stored value (2^-8 for a bf16 gradient, 0 for fp32).  `flush_v` is what flushing
denormals to zero may lose: F32_TINY (the smallest normal fp32 / bf16 number) for the stored value, and scale_v evaluated
at p_v = F32_TINY for the probability itself, which the hardware exp2 returns as 0 below that
(flush_v = F32_TINY (1 + (|g| + |gH| (|ln p_v| + |H|)) / T)).

Bounds (`DLOGITS_BOUND`, `FWD_BOUND`): for each family of inputs the same metric was computed for the REFERENCE's own
fp32 arithmetic (torch CPU fp32 autograd of reference pipelinerl/finetune/rl/__init__.py:207-233, `reference_fp32`
below) against the fp64 witness on the same inputs; the bound is 4 x the largest value in the family (a different
summation order over 152 064 terms, 1-2 ulp of the hardware exp2 / log2) and stays below 5e-4 so that a softmax body
scaled by 1.001 (~1e-3) is still rejected.  No bound comes from a kernel.  tests/test_grad_checks_host.py re-measures the
reference on the CPU and fails if its value exceeds the one written here; DESIGN.md section 7 holds the table.
"""

from __future__ import annotations

import dataclasses
import re

import numpy as np
import torch

F32_TINY = float(np.finfo(np.float32).tiny)
BF16_ROUNDING = 2.0 ** -8  # |round_bf16(x) - x| <= half an ulp = 2^-8 * 2^floor(log2 |x|) <= 2^-8 |x|
MUTANT_FLOOR = 5e-4        # no d logits bound may reach this: "softmax body x 1.001" scores ~1e-3

# family -> largest value of the metric for the reference's fp32 arithmetic, measured on the CPU over every GPU case of
# the family (fp32 and bf16-rounded inputs), rounded up to two digits; bound = 4 x that.
DLOGITS_REF = {
    "randn_spiky": 4.2e-6,   # 2 * randn + one spiky row, the loss configs of test_gpu_fullvocab (V = 4099 .. 152 064)
    "randn": 1.9e-6,         # 2 * randn rows (padded strides, rows x cols, many rows), V = 4099 .. 152 064
    "k1_random_g": 1.9e-6,   # 2 * randn, g ~ N(0, 1), gH ~ 0.1 N(0, 1), temperature 0.8 / 1.0, V = 1031 .. 152 064
    "edges": 4.6e-6,         # label / maximum (+10) / tied maxima at region edges over 2 * randn, temperature 0.7
    "trained": 9.7e-6,       # p(label) ~ 1, offsets +-30, uniform row, 1000 entries at -1e4; temperature 0.3 / 0.7 / 2.0
    "offset_1000": 2.9e-5,   # common offset +-1000 at temperature 1
}
DLOGITS_BOUND = {k: 4.0 * v for k, v in DLOGITS_REF.items()}
assert max(DLOGITS_BOUND.values()) < MUTANT_FLOOR

# largest absolute error (nats) of new_logprobs / entropy / logsumexp of the reference's fp32 path against fp64
FWD_REF = {"randn_spiky": 7.5e-6, "randn": 7.4e-6, "k1_random_g": 7.4e-6, "edges": 6.0e-6, "trained": 1.08e-5,
           "offset_1000": 2.04e-4}
FWD_BOUND = {k: 4.0 * v for k, v in FWD_REF.items()}

# |sum_v d logit_v| / sum_v |d logit_v| of a row (exactly 0 in exact arithmetic when gH = 0): 4.1e-7 for the reference's
# fp32 arithmetic on 256 rows of 2 * randn at V = 152 064, temperature 1
ROWSUM_REF = 4.1e-7
ROWSUM_BOUND = 4.0 * ROWSUM_REF


# ---- kernel regions -------------------------------------------------------------------------------------------------
_NV = {"F32": 4, "BF16": 8}


def parse_kernel(name: str) -> dict:
    """Launch constants out of `prl_last_fused_kernel()`:
    fused_logits_loss_keep_kernel<T,BLOCK,UNROLL,KREG,KLDS,NTHEAD> or fused_logits_loss_kernel<T,BLOCK,UNROLL,REVERSE,NT>."""
    m = re.fullmatch(r"(\w+)<(\w+),(\d+),(\d+),(\w+),(\w+)(?:,(\w+))?>", name)
    if not m:
        raise ValueError(f"unrecognised kernel name {name!r}")
    kind, t, block, unroll = m.group(1), m.group(2), int(m.group(3)), int(m.group(4))
    out = {"kind": kind, "dtype": t, "nv": _NV[t], "block": block, "unroll": unroll, "kreg": 0, "klds": 0}
    if kind == "fused_logits_loss_keep_kernel":
        out.update(kreg=int(m.group(5)), klds=int(m.group(6)))
    elif kind != "fused_logits_loss_kernel":
        raise ValueError(f"unrecognised kernel name {name!r}")
    return out


def kernel_regions(vocab: int, nv: int, block: int, unroll: int, kreg: int = 0, klds: int = 0, vec_ok: bool = True):
    """Column ranges [lo, hi) a row is split into by a logits kernel, in row order, empty ones dropped.
    Row-resident kernel (kreg + klds > 0): register head, LDS head, streamed full tiles, vector tail, scalar tail.
    Two-sweep kernels: full tiles of block * unroll vectors, vector tail, scalar tail (the whole row when the row
    stride or a base pointer breaks 16-byte alignment)."""
    if not vec_ok:
        return [("scalar_tail", 0, vocab)]
    nvec = vocab // nv
    head_reg, head = kreg * block, (kreg + klds) * block
    if nvec < head:
        raise ValueError("row shorter than the on-chip head")
    tile = block * unroll
    nfull = ((nvec - head) // tile) * tile
    cuts = [("register_head", 0, head_reg), ("lds_head", head_reg, head), ("full_tiles", head, head + nfull),
            ("vector_tail", head + nfull, nvec)]
    out = [(n, lo * nv, hi * nv) for n, lo, hi in cuts if hi > lo]
    if vocab > nvec * nv:
        out.append(("scalar_tail", nvec * nv, vocab))
    return out


def regions_of_kernel(name: str, vocab: int, vec_ok: bool = True):
    k = parse_kernel(name)
    return kernel_regions(vocab, k["nv"], k["block"], k["unroll"], k["kreg"], k["klds"], vec_ok)


def region_name(regions, col: int) -> str:
    for n, lo, hi in regions or ():
        if lo <= col < hi:
            return f"{n}[{lo},{hi})"
    return "?"


# ---- fp64 witnesses ---------------------------------------------------------------------------------------------------
def _as_t(a, dtype=None) -> torch.Tensor:
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    t = t.detach().cpu()
    return t if dtype is None else t.to(dtype)


def forward_witness(logits, ids, temperature: float, row_block: int = 32):
    """fp64 (new_logprob, entropy, logsumexp in nats) of every row of `logits` [R, V] for labels `ids` [R]
    (an id outside [0, V) gives a NaN log-prob, as the kernels do)."""
    x, ids = _as_t(logits), _as_t(ids, torch.int64)
    R, V = x.shape
    nlp, ent, lse = (np.zeros(R) for _ in range(3))
    for a in range(0, R, row_block):
        b = slice(a, min(a + row_block, R))
        z = x[b].double() / temperature
        l = torch.logsumexp(z, -1)
        logp = z - l[:, None]
        ent[b] = (-(logp.exp() * logp).sum(-1)).numpy()
        lse[b] = l.numpy()
        i = ids[b]
        ok = (i >= 0) & (i < V)
        sel = logp.gather(1, i.clamp(0, V - 1)[:, None])[:, 0]
        nlp[b] = torch.where(ok, sel, torch.full_like(sel, float("nan"))).numpy()
    return nlp, ent, lse


def _witness_block(x, ids, g, gh, temperature):
    """(want, scale, flush) fp64 [r, V] for a block of rows."""
    V = x.shape[1]
    z = x.double() / temperature
    logp = torch.log_softmax(z, -1)
    p = logp.exp()
    H = -(p * logp).sum(-1, keepdim=True)
    g, gh = g[:, None], gh[:, None]
    want = (-g) * p - gh * p * (logp + H)
    coef = g.abs() + gh.abs() * (logp.abs() + H.abs())
    scale = coef * p
    flush = F32_TINY * (1.0 + coef / temperature)
    rows = torch.arange(x.shape[0], device=x.device)
    ok = (ids >= 0) & (ids < V)
    want[rows[ok], ids[ok]] += g[ok, 0]
    scale[rows[ok], ids[ok]] += g[ok, 0].abs()
    dead = ((g == 0) & (gh == 0)).expand_as(want)  # 0 * NaN of a row that is never read must not leak in
    want[dead] = 0.0
    scale[dead] = 0.0
    return want / temperature, scale / temperature, flush


def dlogits_witness(logits, ids, g_nlp, g_ent, temperature: float, row_block: int = 16):
    """fp64 closed form of d logits, the size of its terms before they cancel and the flush allowance, each [R, V] numpy.
    `logits` [R, V] (any float dtype, used as stored), `ids` [R] the label of each row, `g_nlp` / `g_ent` [R]."""
    x, ids = _as_t(logits), _as_t(ids, torch.int64)
    g, gh = _as_t(g_nlp, torch.float64), _as_t(g_ent, torch.float64)
    R, V = x.shape
    want, scale, flush = np.empty((R, V)), np.empty((R, V)), np.empty((R, V))
    for a in range(0, R, row_block):
        b = slice(a, min(a + row_block, R))
        w, s, f = _witness_block(x[b], ids[b], g[b], gh[b], temperature)
        want[b], scale[b], flush[b] = w.numpy(), s.numpy(), f.numpy()
    return want, scale, flush


@dataclasses.dataclass
class GradCheck:
    err: float          # max over entries with scale > 0 of the excess error / scale
    row: int
    col: int
    region: str
    got: float
    want: float
    scale: float
    stray: int          # non-zero entries where scale == 0 (must be 0)
    stray_at: tuple | None

    def __str__(self):
        s = (f"per-entry d logits error {self.err:.3e} at row {self.row} col {self.col} region {self.region}: "
             f"got {self.got:.9e} want {self.want:.9e} scale {self.scale:.3e}")
        if self.stray:
            s += f"; {self.stray} non-zero entries where the gradient is exactly 0, first at {self.stray_at}"
        return s

    def ok(self, bound: float) -> bool:
        return self.stray == 0 and self.err <= bound  # NaN fails


def dlogits_error(got, logits, ids, g_nlp, g_ent, temperature: float, *, out_rounding: float = 0.0, regions=None,
                  witness=None, row_block: int = 16) -> GradCheck:
    """The metric of the module docstring.  `got` [R, V]; the other arguments as in `dlogits_witness`.  `witness`: a
    (want, scale, flush) triple computed earlier for the same inputs (shared between variants); otherwise it is built here in
    blocks of `row_block` rows, so a 64 x 152 064 case needs ~100 MB.  `regions`: `kernel_regions(...)` of the kernel
    that wrote `got`, for the message."""
    got_t = _as_t(got)
    R, V = got_t.shape
    if witness is None:
        x, ids_t = _as_t(logits), _as_t(ids, torch.int64)
        g, gh = _as_t(g_nlp, torch.float64), _as_t(g_ent, torch.float64)
    best = (-1.0, 0, 0)
    stray, stray_at = 0, None
    for a in range(0, R, row_block):
        b = slice(a, min(a + row_block, R))
        if witness is None:
            want, scale, flush = _witness_block(x[b], ids_t[b], g[b], gh[b], temperature)
        else:
            want, scale, flush = (torch.from_numpy(w[b]) for w in witness)
        gb = got_t[b].double()
        live = scale > 0
        bad = ~live & (gb != 0)  # NaN != 0 is true: a NaN in a zero entry is stray too
        n_bad = int(bad.sum())
        if n_bad:
            if stray_at is None:
                r, c = np.argwhere(bad.numpy())[0]
                stray_at = (a + int(r), int(c))
            stray += n_bad
        excess = (gb - want).abs() - out_rounding * want.abs() - flush
        e = torch.where(live, excess.clamp_min(0.0) / torch.where(live, scale, torch.ones_like(scale)), torch.zeros_like(scale))
        e = torch.where(torch.isnan(gb) & live, torch.full_like(e, float("inf")), e)
        m = float(e.max())
        if m > best[0]:
            k = int(e.argmax())
            best = (m, a + k // V, k % V)
    err, r, c = best
    if witness is None:
        w_rc, s_rc, _ = _witness_block(x[r:r + 1], ids_t[r:r + 1], g[r:r + 1], gh[r:r + 1], temperature)
        w_rc, s_rc = float(w_rc[0, c]), float(s_rc[0, c])
    else:
        w_rc, s_rc = float(witness[0][r, c]), float(witness[1][r, c])
    return GradCheck(err, r, c, region_name(regions, c), float(got_t[r, c]), w_rc, s_rc, stray, stray_at)


def token_rows(input_ids, g_nlp_shifted, g_ent_shifted):
    """Row-level (ids, g, gH) of a token-aligned batch: logits row (b, t) predicts input_ids[b, t + 1] with the
    shifted-axis gradients [B, L - 1]; each sequence's last row predicts nothing (g = gH = 0, id = -1)."""
    ids = np.asarray(input_ids)
    B, L = ids.shape
    rid = np.full((B, L), -1, dtype=np.int64)
    rid[:, :-1] = ids[:, 1:]
    g, gh = np.zeros((B, L)), np.zeros((B, L))
    g[:, :-1] = np.asarray(g_nlp_shifted, dtype=np.float64)
    gh[:, :-1] = np.asarray(g_ent_shifted, dtype=np.float64)
    return rid.reshape(-1), g.reshape(-1), gh.reshape(-1)


# ---- the reference's own fp32 arithmetic (the yardstick of every bound) -------------------------------------------------
def reference_fp32(logits, ids, g_nlp, g_ent, temperature: float, row_block: int = 16, hidden=None, weight=None):
    """torch CPU fp32 restatement of reference rl/__init__.py:207-233 with autograd:
    returns (d logits [R, V] fp32, new_logprobs [R], entropy [R], logsumexp [R]) for loss = sum(g nlp + gH entropy).
    With `hidden` [R, H] and `weight` [V, H] (`logits` None) the logits are the reference's fp32 head product
    `hidden.float() @ weight.float().T` (finetune/checkpoints.py:87-103) inside the same graph, and two more values are
    returned: d hidden [R, H] and d weight [V, H], fp32."""
    ids = _as_t(ids, torch.int64)
    g, gh = _as_t(g_nlp, torch.float32), _as_t(g_ent, torch.float32)
    head = hidden is not None
    if head:
        h = _as_t(hidden).float().requires_grad_(True)
        w = _as_t(weight).float().requires_grad_(True)
        R, V = h.shape[0], w.shape[0]
    else:
        x = _as_t(logits).float()
        R, V = x.shape
    grad = np.zeros((R, V), dtype=np.float32)
    nlp, ent, lse = (np.zeros(R, dtype=np.float32) for _ in range(3))
    for a in range(0, R, row_block):
        b = slice(a, min(a + row_block, R))
        if head:
            xb = h[b] @ w.t()
            xb.retain_grad()
        else:
            xb = x[b].clone().requires_grad_(True)
        z = xb / temperature
        sel = torch.gather(z, 1, ids[b].clamp(0, V - 1)[:, None])[:, 0]
        log_norm = torch.logsumexp(z, dim=-1)
        new_lp = sel - log_norm
        logprobs = z - log_norm.unsqueeze(-1)
        probs = torch.exp(logprobs)
        entropy = -(probs * logprobs).sum(dim=-1)
        valid = ((ids[b] >= 0) & (ids[b] < V)).float()
        (new_lp * g[b] * valid + entropy * gh[b]).sum().backward()
        grad[b] = xb.grad.numpy()
        nlp[b], ent[b], lse[b] = new_lp.detach().numpy(), entropy.detach().numpy(), log_norm.detach().numpy()
    if head:
        return grad, nlp, ent, lse, h.grad.numpy(), w.grad.numpy()
    return grad, nlp, ent, lse


def round_bf16(a: np.ndarray) -> np.ndarray:
    """Round-to-nearest-even to bf16, returned as fp32 (what a bf16 gradient buffer holds)."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).float().numpy()
