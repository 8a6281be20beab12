"""Packed variable-length causal attention for the learner body (csrc/prl_attention.hip).

The learner hands the stock transformers body a packed `[1, T]` micro-batch with `attention_mask = ones` and per-sequence
`position_ids`.  Under `attn_implementation="sdpa"` that batch is attended as ONE sequence of T tokens: the tokens of a later
sequence see every earlier one.  The reference keeps packed sequences apart with flash-attn's varlen path, driven by the
`position_ids` resets.  This module is that path:

    segments(position_ids, attention_mask)           the two int32 arrays seq_start / seq_end over the flattened B T tokens
    varlen_attention(q, k, v, seq_start, seq_end, scale)   key j visible to query i iff seq_start[i] <= j <= i; bf16, HIP
    install_fused_attention(model)                   registers "prl_varlen" with transformers' AttentionInterface and
                                                     switches this model to it; opt-in, per model
    varlen_attention_slice(q, k_all, v_all, seq_start, seq_end, q_offset, scale)
                                                     the sequence-parallel form (csrc/prl_attention_sp.hip): the queries of one
                                                     contiguous slice of a packed row against the keys of the whole row
    install_fused_attention(model, seq_parallel_group=g)   every rank of g holds one `make_slices` slice: K / V and the segment
                                                     table are gathered over g, the fp32 dK / dV partials exchanged and folded

The kernels read only the key blocks from a query block's sequence start to its diagonal, so a batch of 8 x 1024 tokens does
about 1/8 of the matrix work of one 8192-token sequence and nothing of size T x T is ever written.  Backward is three launches
without atomics: two runs give the same bits.

Anything the kernels do not take (CPU tensors, fp32 / fp16, a head size other than 64 / 128, dropout, a sliding window, a
soft-cap) goes to transformers' `sdpa_attention_forward` under a block-diagonal causal bool mask built from the SAME segment
table - O(T^2), on that fallback only - so an installed model keeps packed sequences apart on every path.
"""

from __future__ import annotations

import ctypes
from typing import Any

import torch
from torch.autograd.function import once_differentiable

from . import _lib
from .fused_body import _fn, _launch

NAME = "prl_varlen"
BQ = 64  # query rows of a workgroup's block      (PRL_ATTN_BQ of csrc/prl_attention.hip; tests/test_attention_api.py compares)
BK = 64  # keys of one swept tile / of a dK, dV block  (PRL_ATTN_BK)
HEAD_SIZES = (64, 128)

_CACHE_ENTRIES = 4
_seg_cache: list[tuple] = []  # (position_ids, its _version, attention_mask, its _version, shape, seq_start, seq_end), newest last
_ws_bytes: dict[tuple[int, int], int] = {}
_sp_cache: list[tuple] = []  # (group, position_ids, its _version, attention_mask, its _version, shape, seq_start, seq_end) of the GATHERED row
_sp_ws_bytes: dict[tuple[int, int], int] = {}


# ---- segment table -----------------------------------------------------------------------------------------------------------
def _segments_torch(position_ids, attention_mask, batch: int, t: int, device) -> tuple[torch.Tensor, torch.Tensor]:
    """The rule of `prl_attn_segments` in plain torch: the witness of the kernel and the basis of the fallback."""
    n = batch * t
    idx = torch.arange(n, device=device, dtype=torch.int64).view(batch, t)
    start = torch.zeros(batch, t, dtype=torch.bool, device=device)
    if t:
        start[:, 0] = True
    if position_ids is not None:
        start[:, 1:] |= position_ids[:, 1:] != position_ids[:, :-1] + 1
    if attention_mask is not None:
        zero = attention_mask == 0
        start[:, 1:] |= zero[:, 1:] | zero[:, :-1]
    seq_start = torch.where(start, idx, torch.full_like(idx, -1)).cummax(dim=1).values
    row_end = (torch.arange(batch, device=device, dtype=torch.int64).view(batch, 1) + 1) * t
    nxt = torch.where(start, idx, row_end.expand(batch, t))
    nxt = torch.cat([nxt[:, 1:], row_end], dim=1)  # the candidates after token c
    seq_end = nxt.flip(1).cummin(dim=1).values.flip(1)
    return seq_start.reshape(n).to(torch.int32), seq_end.reshape(n).to(torch.int32)


def segments(position_ids: torch.Tensor | None = None, attention_mask: torch.Tensor | None = None,
             shape: tuple[int, int] | None = None) -> tuple[torch.Tensor, torch.Tensor]:
    """`(seq_start, seq_end)`, int32 `[B * T]`: for every token of a `[B, T]` batch the flat index of the first token of its
    sequence and one past its last.  Token `b T + c` starts a sequence iff `c == 0`, or `position_ids[b, c] !=
    position_ids[b, c - 1] + 1` (transformers' `find_packed_sequence_indices`), or the 2-D `attention_mask` is 0 at `c` or at
    `c - 1`: every pad token is a sequence of length 1, the real tokens of a left- or right-padded row are one sequence.
    `shape` is needed when both are None.  On a HIP device this is one launch and no copy to the host; on the CPU plain torch."""
    ref = position_ids if position_ids is not None else attention_mask
    if shape is None:
        if ref is None:
            raise ValueError("segments() needs position_ids, attention_mask or shape")
        shape = (int(attention_mask.shape[0]), int(attention_mask.shape[1])) if attention_mask is not None else tuple(int(s) for s in position_ids.shape)
    batch, t = int(shape[0]), int(shape[1])
    if attention_mask is not None and (attention_mask.dim() != 2 or tuple(attention_mask.shape) != (batch, t)):
        raise ValueError(f"attention_mask {tuple(attention_mask.shape)} is not the 2-D mask of a [{batch}, {t}] batch")
    if position_ids is not None:
        if position_ids.dim() != 2 or position_ids.shape[1] != t or position_ids.shape[0] not in (1, batch):
            raise ValueError(f"position_ids {tuple(position_ids.shape)} do not belong to a [{batch}, {t}] batch")
        if position_ids.shape[0] != batch:
            position_ids = position_ids.expand(batch, t)
    if ref is None or not ref.is_cuda:
        return _segments_torch(position_ids, attention_mask, batch, t, ref.device if ref is not None else torch.device("cpu"))
    device = ref.device
    pos = mask = None
    mask_bytes = 0
    if position_ids is not None:
        pos = position_ids.to(device=device, dtype=torch.int64).contiguous()
    if attention_mask is not None:
        mask = attention_mask.to(device)
        if mask.dtype not in (torch.bool, torch.uint8, torch.int8, torch.int32, torch.int64):
            mask = mask != 0
        mask = mask.contiguous()
        mask_bytes = mask.element_size()
    seq_start = torch.empty(batch * t, dtype=torch.int32, device=device)
    seq_end = torch.empty(batch * t, dtype=torch.int32, device=device)
    _launch("prl_attn_segments", device, batch, t, _lib.ptr(pos), _lib.ptr(mask), mask_bytes, seq_start.data_ptr(), seq_end.data_ptr())
    return seq_start, seq_end


def _cached_segments(position_ids, attention_mask, shape) -> tuple[torch.Tensor, torch.Tensor]:
    """One table per model forward: every layer of a forward gets the same `position_ids` / mask objects."""
    pv = position_ids._version if position_ids is not None else -1
    mv = attention_mask._version if attention_mask is not None else -1
    for e in reversed(_seg_cache):
        if e[0] is position_ids and e[2] is attention_mask and e[1] == pv and e[3] == mv and e[4] == shape:
            return e[5], e[6]
    seq_start, seq_end = segments(position_ids, attention_mask, shape)
    _seg_cache.append((position_ids, pv, attention_mask, mv, shape, seq_start, seq_end))
    del _seg_cache[:-_CACHE_ENTRIES]
    return seq_start, seq_end


# ---- the op --------------------------------------------------------------------------------------------------------------------
def _workspace_bytes(n: int, hq: int) -> int:
    need = _ws_bytes.get((n, hq))
    if need is None:
        out = ctypes.c_size_t(0)
        _lib.check(_fn("prl_attn_workspace_bytes")(n, hq, ctypes.byref(out)))
        if len(_ws_bytes) > 4096:
            _ws_bytes.clear()
        need = _ws_bytes[(n, hq)] = out.value
    return need


def _rows_ok(x: torch.Tensor) -> bool:
    return x.stride(2) == 1 and x.stride(0) % 8 == 0 and x.stride(1) % 8 == 0 and x.stride(0) >= x.shape[2] and x.data_ptr() % 16 == 0


def _operand(x: torch.Tensor) -> torch.Tensor:
    """[N, H, D] as the kernels read it: D contiguous, rows 16-byte aligned, any token / head stride; else one copy."""
    return x if _rows_ok(x) else x.contiguous()


class _VarlenAttnFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, seq_start, seq_end, scale):  # type: ignore[override]
        for t in (q, k, v, seq_start, seq_end):
            if not t.is_cuda:
                _lib.require_device(t)
        if q.dtype != torch.bfloat16 or k.dtype != torch.bfloat16 or v.dtype != torch.bfloat16:
            raise TypeError(f"the attention kernels take bf16 q, k, v, not {q.dtype} / {k.dtype} / {v.dtype}")
        if q.dim() != 3 or k.dim() != 3 or v.shape != k.shape or k.shape[0] != q.shape[0] or k.shape[2] != q.shape[2]:
            raise ValueError(f"q {tuple(q.shape)}, k {tuple(k.shape)}, v {tuple(v.shape)} are not [N, Hq, D], [N, Hkv, D], [N, Hkv, D]")
        n, hq, d = q.shape
        hkv = k.shape[1]
        if seq_start.dtype != torch.int32 or seq_end.dtype != torch.int32 or seq_start.numel() != n or seq_end.numel() != n:
            raise ValueError(f"seq_start / seq_end must be int32 [{n}] (segments())")
        qc, kc, vc = _operand(q), _operand(k), _operand(v)
        ss, se = seq_start.contiguous(), seq_end.contiguous()
        out = torch.empty((n, hq, d), dtype=torch.bfloat16, device=q.device)
        lse = torch.empty((hq, n), dtype=torch.float32, device=q.device)
        _launch("prl_attn_varlen_fwd", q.device, n, hq, hkv, d, qc.data_ptr(), qc.stride(0), qc.stride(1), kc.data_ptr(), kc.stride(0), kc.stride(1),
                vc.data_ptr(), vc.stride(0), vc.stride(1), float(scale), ss.data_ptr(), se.data_ptr(), out.data_ptr(), lse.data_ptr())
        ctx.save_for_backward(qc, kc, vc, out, lse)
        ctx.table = (ss, se)  # (int32 indices, no gradient: the per-forward table every layer shares)
        ctx.scale = float(scale)
        ctx.mark_non_differentiable(lse)
        return out, lse

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out, _grad_lse):  # type: ignore[override]
        qc, kc, vc, out, lse = ctx.saved_tensors
        ss, se = ctx.table
        n, hq, d = qc.shape
        hkv = kc.shape[1]
        g = grad_out.contiguous()
        if g.data_ptr() % 16:  # (a contiguous slice of a flat buffer: the kernels read whole 16-byte pieces of rows)
            g = g.clone()
        dq = torch.empty((n, hq, d), dtype=torch.bfloat16, device=qc.device)
        dk = torch.empty((n, hkv, d), dtype=torch.bfloat16, device=qc.device)
        dv = torch.empty((n, hkv, d), dtype=torch.bfloat16, device=qc.device)
        ws_bytes = _workspace_bytes(n, hq)
        ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=qc.device)
        _launch("prl_attn_varlen_bwd", qc.device, n, hq, hkv, d, qc.data_ptr(), qc.stride(0), qc.stride(1), kc.data_ptr(), kc.stride(0), kc.stride(1),
                vc.data_ptr(), vc.stride(0), vc.stride(1), ctx.scale, ss.data_ptr(), se.data_ptr(), out.data_ptr(), lse.data_ptr(), g.data_ptr(),
                dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), ws.data_ptr(), ws_bytes)
        return dq, dk, dv, None, None, None


def varlen_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, seq_start: torch.Tensor, seq_end: torch.Tensor, scale: float,
                     return_lse: bool = False):
    """Causal attention inside the sequences of a packed batch: bf16 `q [N, Hq, D]`, `k, v [N, Hkv, D]` on a HIP device
    (D = 64 or 128 contiguous, `Hq % Hkv == 0`, any token / head stride that keeps rows 16-byte aligned; anything else is copied
    once), `seq_start` / `seq_end` from `segments()`.  Returns `out [N, Hq, D]` in bf16, and with `return_lse` the fp32
    `lse [Hq, N]` = ln sum_j exp(scale q_i . k_j) over the visible keys.  Differentiable in q, k, v; saves q, k, v, out and lse
    (plus a reference to the shared segment table).  Raises on CPU tensors: there is no fallback here."""
    out, lse = _VarlenAttnFn.apply(q, k, v, seq_start, seq_end, scale)
    return (out, lse) if return_lse else out


# ---- the sequence-parallel slice op ----------------------------------------------------------------------------------------------
def _slice_workspace_bytes(nq: int, hq: int) -> int:
    need = _sp_ws_bytes.get((nq, hq))
    if need is None:
        out = ctypes.c_size_t(0)
        _lib.check(_fn("prl_attn_slice_workspace_bytes")(nq, hq, ctypes.byref(out)))
        if len(_sp_ws_bytes) > 4096:
            _sp_ws_bytes.clear()
        need = _sp_ws_bytes[(nq, hq)] = out.value
    return need


def _check_slice(q, k_all, v_all, seq_start, seq_end, q_offset: int) -> None:
    for t in (q, k_all, v_all, seq_start, seq_end):
        if not t.is_cuda:
            _lib.require_device(t)
    if q.dtype != torch.bfloat16 or k_all.dtype != torch.bfloat16 or v_all.dtype != torch.bfloat16:
        raise TypeError(f"the attention kernels take bf16 q, k, v, not {q.dtype} / {k_all.dtype} / {v_all.dtype}")
    if q.dim() != 3 or k_all.dim() != 3 or v_all.shape != k_all.shape or k_all.shape[2] != q.shape[2]:
        raise ValueError(f"q {tuple(q.shape)}, k_all {tuple(k_all.shape)}, v_all {tuple(v_all.shape)} are not [nq, Hq, D], [nk, Hkv, D], [nk, Hkv, D]")
    nq, nk = q.shape[0], k_all.shape[0]
    if isinstance(q_offset, bool) or not isinstance(q_offset, int):
        raise TypeError(f"q_offset must be an int, not {type(q_offset).__name__}")
    if q_offset < 0 or q_offset + nq > nk:
        raise ValueError(f"q_offset {q_offset}: the {nq} local queries must lie inside the {nk} keys of the gathered row")
    if seq_start.dtype != torch.int32 or seq_end.dtype != torch.int32 or seq_start.numel() != nk or seq_end.numel() != nk:
        raise ValueError(f"seq_start / seq_end must be int32 [{nk}]: segments() of the WHOLE gathered row")


def _slice_forward(qc, kc, vc, ss, se, q_offset: int, scale: float) -> tuple[torch.Tensor, torch.Tensor]:
    nq, hq, d = qc.shape
    nk, hkv = kc.shape[0], kc.shape[1]
    out = torch.empty((nq, hq, d), dtype=torch.bfloat16, device=qc.device)
    lse = torch.empty((hq, nq), dtype=torch.float32, device=qc.device)
    if nq:
        _launch("prl_attn_slice_fwd", qc.device, nq, nk, q_offset, hq, hkv, d, qc.data_ptr(), qc.stride(0), qc.stride(1), kc.data_ptr(), kc.stride(0),
                kc.stride(1), vc.data_ptr(), vc.stride(0), vc.stride(1), float(scale), ss.data_ptr(), se.data_ptr(), out.data_ptr(), lse.data_ptr())
    return out, lse


def _slice_backward(qc, kc, vc, ss, se, q_offset: int, scale: float, out, lse, grad_out):
    """(grad_q bf16 [nq, Hq, D], grad_k_part, grad_v_part fp32 [nk, Hkv, D]): every element of the partials is defined."""
    nq, hq, d = qc.shape
    nk, hkv = kc.shape[0], kc.shape[1]
    dq = torch.empty((nq, hq, d), dtype=torch.bfloat16, device=qc.device)
    if not nq:
        z = torch.zeros((nk, hkv, d), dtype=torch.float32, device=qc.device)
        return dq, z, torch.zeros_like(z)
    g = grad_out.contiguous()
    if g.data_ptr() % 16:  # (a contiguous slice of a flat buffer: the kernels read whole 16-byte pieces of rows)
        g = g.clone()
    dkp = torch.empty((nk, hkv, d), dtype=torch.float32, device=qc.device)
    dvp = torch.empty((nk, hkv, d), dtype=torch.float32, device=qc.device)
    ws_bytes = _slice_workspace_bytes(nq, hq)
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=qc.device)
    _launch("prl_attn_slice_bwd", qc.device, nq, nk, q_offset, hq, hkv, d, qc.data_ptr(), qc.stride(0), qc.stride(1), kc.data_ptr(), kc.stride(0),
            kc.stride(1), vc.data_ptr(), vc.stride(0), vc.stride(1), float(scale), ss.data_ptr(), se.data_ptr(), out.data_ptr(), lse.data_ptr(),
            g.data_ptr(), dq.data_ptr(), dkp.data_ptr(), dvp.data_ptr(), ws.data_ptr(), ws_bytes)
    return dq, dkp, dvp


def fold_parts(parts: torch.Tensor) -> torch.Tensor:
    """fp32 `parts [P, ...]` -> bf16 `[...]`: `rne(parts[0] + parts[1] + ... + parts[P - 1])`, the sum in fp32 in rank order, one
    rounding.  One launch on a HIP device; the same order in plain torch on the CPU."""
    if parts.dtype != torch.float32 or parts.dim() < 1 or parts.shape[0] < 1:
        raise ValueError(f"fold_parts takes fp32 [P, ...] with P >= 1, not {parts.dtype} {tuple(parts.shape)}")
    if not parts.is_cuda:
        acc = parts[0].clone()
        for r in range(1, parts.shape[0]):
            acc = acc + parts[r]
        return acc.to(torch.bfloat16)
    pc = parts.contiguous()
    if pc.data_ptr() % 16:
        pc = pc.clone()
    out = torch.empty(pc.shape[1:], dtype=torch.bfloat16, device=pc.device)
    _launch("prl_attn_fold_parts", pc.device, pc.shape[0], out.numel(), pc.data_ptr(), out.data_ptr())
    return out


class _SliceAttnFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k_all, v_all, seq_start, seq_end, q_offset, scale, sink):  # type: ignore[override]
        _check_slice(q, k_all, v_all, seq_start, seq_end, q_offset)
        qc, kc, vc = _operand(q), _operand(k_all), _operand(v_all)
        ss, se = seq_start.contiguous(), seq_end.contiguous()
        out, lse = _slice_forward(qc, kc, vc, ss, se, q_offset, scale)
        ctx.save_for_backward(qc, kc, vc, out, lse)
        ctx.table, ctx.q_offset, ctx.scale, ctx.sink = (ss, se), q_offset, float(scale), sink
        ctx.mark_non_differentiable(lse)
        return out, lse

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out, _grad_lse):  # type: ignore[override]
        qc, kc, vc, out, lse = ctx.saved_tensors
        dq, dkp, dvp = _slice_backward(qc, kc, vc, *ctx.table, ctx.q_offset, ctx.scale, out, lse, grad_out)
        if ctx.sink is not None:
            ctx.sink.append((dkp, dvp))
        return dq, None, None, None, None, None, None, None


def varlen_attention_slice(q: torch.Tensor, k_all: torch.Tensor, v_all: torch.Tensor, seq_start: torch.Tensor, seq_end: torch.Tensor, q_offset: int,
                           scale: float, return_lse: bool = False, kv_grad_parts: list | None = None):
    """The sequence-parallel form of `varlen_attention`, in one process: bf16 `q [nq, Hq, D]` are the queries of the contiguous
    slice `[q_offset, q_offset + nq)` of a packed row, `k_all`, `v_all [nk, Hkv, D]` and `seq_start` / `seq_end` (`segments()`
    of the gathered row) cover the WHOLE row.  Key j is visible to local query i iff `seq_start[q_offset + i] <= j <= q_offset
    + i`.  Returns `out [nq, Hq, D]` in bf16, and with `return_lse` the fp32 `lse [Hq, nq]`.  Differentiable in `q`.  The
    gradients of `k_all` / `v_all` are this slice's SHARE of sums over all slices, so they do not flow into `k_all.grad` (autograd
    would round them to bf16, once per slice): pass a list as `kv_grad_parts` and the backward appends `(grad_k_part, grad_v_part)`,
    fp32 `[nk, Hkv, D]` with exact zeros in the rows no local query sees; `fold_parts(torch.stack(parts of all slices, in slice
    order))` is the bf16 gradient of the whole row.  With `q_offset` a multiple of 64 out, lse and grad_q are the rows of the
    square op on the whole row bit for bit.  Raises on CPU tensors."""
    out, lse = _SliceAttnFn.apply(q, k_all, v_all, seq_start, seq_end, q_offset, scale, kv_grad_parts)
    return (out, lse) if return_lse else out


# ---- collectives of a sequence-parallel group ----------------------------------------------------------------------------------
def _group_size(group) -> int:
    import torch.distributed as dist

    if group is None or not (dist.is_available() and dist.is_initialized()):
        return 1
    return dist.get_world_size(group)


def _gather_rows(x: torch.Tensor, group) -> torch.Tensor:
    """`[L, ...]` of every rank -> `[P L, ...]` in rank order (bytes: any dtype travels over any backend)."""
    import torch.distributed as dist

    p = dist.get_world_size(group)
    send = x.contiguous().view(-1).view(torch.uint8)
    recv = torch.empty(p * send.numel(), dtype=torch.uint8, device=x.device)
    if dist.get_backend(group) == "nccl":
        dist.all_gather_into_tensor(recv, send, group=group)
    else:
        dist.all_gather(list(recv.view(p, -1).unbind(0)), send, group=group)
    return recv.view(x.dtype).view((p * x.shape[0],) + tuple(x.shape[1:]))


def _exchange_rows(parts: torch.Tensor, group) -> torch.Tensor:
    """`parts [P L, ...]`, this rank's share of a sum over the whole row -> `[P, L, ...]`: piece r is rank r's share of THIS
    rank's rows.  One `all_to_all_single`: rank r sends rank s the rows `[s L, (s + 1) L)`."""
    import torch.distributed as dist

    p = dist.get_world_size(group)
    send = parts.contiguous()
    recv = torch.empty_like(send)
    dist.all_to_all_single(recv, send, group=group)
    return recv.view((p, send.shape[0] // p) + tuple(send.shape[1:]))


class _SpAttnFn(torch.autograd.Function):
    """Gather K / V over the group, the slice op at `rank L`, and in backward the exchange and fold of the fp32 partials."""

    @staticmethod
    def forward(ctx, q, k, v, seq_start, seq_end, scale, group):  # type: ignore[override]
        import torch.distributed as dist

        if k.dtype != torch.bfloat16 or v.dtype != torch.bfloat16 or k.dim() != 3 or v.shape != k.shape or k.shape[0] != q.shape[0]:
            raise ValueError(f"q {tuple(q.shape)}, k {tuple(k.shape)}, v {tuple(v.shape)} are not the bf16 [L, Hq, D], [L, Hkv, D], [L, Hkv, D] of one slice")
        q_offset = dist.get_rank(group) * q.shape[0]
        k_all, v_all = _gather_rows(k, group), _gather_rows(v, group)
        _check_slice(q, k_all, v_all, seq_start, seq_end, q_offset)
        qc = _operand(q)
        ss, se = seq_start.contiguous(), seq_end.contiguous()
        out, lse = _slice_forward(qc, k_all, v_all, ss, se, q_offset, scale)
        ctx.save_for_backward(qc, k_all, v_all, out, lse)  # the gathered K / V are saved: 2 x P L Hkv D bf16 per layer
        ctx.table, ctx.q_offset, ctx.scale, ctx.group = (ss, se), q_offset, float(scale), group
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):  # type: ignore[override]
        qc, k_all, v_all, out, lse = ctx.saved_tensors
        dq, dkp, dvp = _slice_backward(qc, k_all, v_all, *ctx.table, ctx.q_offset, ctx.scale, out, lse, grad_out)
        dk = fold_parts(_exchange_rows(dkp, ctx.group))  # K first, then V: every rank issues the collectives in this order
        dv = fold_parts(_exchange_rows(dvp, ctx.group))
        return dq, dk, dv, None, None, None, None


class _GatherRowsFn(torch.autograd.Function):
    """The fallback's all-gather: `[L, ...]` -> `[P L, ...]`; backward sums the P ranks' gradients of this rank's rows in rank order
    (in fp32 at least), the same exchange as the kernels' partials."""

    @staticmethod
    def forward(ctx, x, group):  # type: ignore[override]
        ctx.group, ctx.dtype = group, x.dtype
        return _gather_rows(x, group)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):  # type: ignore[override]
        wide = grad if grad.dtype in (torch.float32, torch.float64) else grad.float()
        pieces = _exchange_rows(wide, ctx.group)
        acc = pieces[0].clone()
        for r in range(1, pieces.shape[0]):
            acc = acc + pieces[r]
        return acc.to(ctx.dtype), None


def _sp_segments(position_ids, attention_mask, shape, group, device):
    """The segment table of the gathered row, once per model forward: `position_ids` / the 2-D mask of the slices are gathered over
    the group and `segments()` runs on the whole `[1, P L]` row - only global column 0 starts a sequence unconditionally, a sequence
    that crosses a cut is one sequence.  Slices of unequal length raise."""
    import torch.distributed as dist

    pv = position_ids._version if position_ids is not None else -1
    mv = attention_mask._version if attention_mask is not None else -1
    for e in reversed(_sp_cache):
        if e[0] is group and e[1] is position_ids and e[3] is attention_mask and e[2] == pv and e[4] == mv and e[5] == shape:
            return e[6], e[7]
    batch, t = shape
    if batch != 1:
        raise NotImplementedError(f"sequence-parallel attention takes one packed row per rank ([1, L] slices of make_slices), not a batch of {batch}")
    p = dist.get_world_size(group)
    lengths = _gather_rows(torch.tensor([t, int(position_ids is not None), int(attention_mask is not None)], dtype=torch.int64, device=device), group)
    lengths = lengths.view(p, 3).tolist()
    if any(row != lengths[0] for row in lengths):
        raise ValueError(f"sequence-parallel attention needs slices of equal length and kind on every rank of the group (make_slices); the ranks "
                         f"hold (length, has position_ids, has attention_mask) = {lengths}")
    pos_all = mask_all = None
    if position_ids is not None:
        pos_all = _gather_rows(position_ids[:1].to(device=device, dtype=torch.int64).reshape(t), group).view(1, p * t)
    if attention_mask is not None:
        mask_all = _gather_rows((attention_mask != 0).to(device=device, dtype=torch.uint8).reshape(t), group).view(1, p * t)
    seq_start, seq_end = segments(pos_all, mask_all, (1, p * t))
    _sp_cache.append((group, position_ids, pv, attention_mask, mv, shape, seq_start, seq_end))
    del _sp_cache[:-_CACHE_ENTRIES]
    return seq_start, seq_end


def _sp_attention_forward(module, group, query, key, value, attention_mask, position_ids, dropout, scaling, sliding_window, softcap, kwargs):
    """"prl_varlen" on one slice of a row whose other slices the ranks of `group` hold."""
    import torch.distributed as dist

    batch, hq, t, d = query.shape
    p, rank = dist.get_world_size(group), dist.get_rank(group)
    seq_start, seq_end = _sp_segments(position_ids, attention_mask, (batch, t), group, query.device)
    position_bias = kwargs.get("position_bias")
    kernel = (query.is_cuda and query.dtype == torch.bfloat16 and key.dtype == torch.bfloat16 and value.dtype == torch.bfloat16 and d in HEAD_SIZES
              and not dropout and sliding_window is None and softcap is None and position_bias is None and hq % key.shape[1] == 0)
    if kernel:
        qf = query.transpose(1, 2).reshape(t, hq, d)
        kf = key.transpose(1, 2).reshape(t, key.shape[1], d)
        vf = value.transpose(1, 2).reshape(t, value.shape[1], d)
        out = seq_parallel_attention(qf, kf, vf, seq_start, seq_end, scaling, group)
        return out.view(batch, t, hq, d), None
    from transformers.integrations.sdpa_attention import sdpa_attention_forward

    k_all = _GatherRowsFn.apply(key[0].transpose(0, 1), group).transpose(0, 1).unsqueeze(0)  # [1, Hkv, P L, D]
    v_all = _GatherRowsFn.apply(value[0].transpose(0, 1), group).transpose(0, 1).unsqueeze(0)
    mask = block_diagonal_mask(seq_start.to(query.device), 1, p * t)[:, :, rank * t:(rank + 1) * t, :]  # the [L, P L] rectangle of this slice
    if sliding_window is not None:
        i = torch.arange(rank * t, (rank + 1) * t, device=query.device).view(t, 1)
        j = torch.arange(p * t, device=query.device).view(1, p * t)
        mask = mask & (i - j < sliding_window)
    extra = {k_: v_ for k_, v_ in kwargs.items() if k_ != "position_ids"}
    if softcap is not None:
        extra["softcap"] = softcap
    return sdpa_attention_forward(module, query, k_all, v_all, mask, dropout=dropout, scaling=scaling, is_causal=False, **extra)


def seq_parallel_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, seq_start: torch.Tensor, seq_end: torch.Tensor, scale: float, group):
    """The kernels' path of an installed model under a group, as an op: bf16 `q [L, Hq, D]`, `k, v [L, Hkv, D]` of THIS rank's slice
    (every rank holds L tokens), `seq_start` / `seq_end` of the gathered `[P L]` row.  All-gathers k, v over `group`, runs the slice
    op at `rank L`, and in backward exchanges the fp32 partials (one `all_to_all_single` per tensor) and folds them in rank order:
    differentiable in q, k, v.  Saves q, out, lse and the gathered K / V."""
    return _SpAttnFn.apply(q, k, v, seq_start, seq_end, scale, group)


# ---- transformers integration ------------------------------------------------------------------------------------------------
def block_diagonal_mask(seq_start: torch.Tensor, batch: int, t: int) -> torch.Tensor:
    """bool `[B, 1, T, T]`, True where key j is visible to query i: the dense form of the segment table (fallback and tests)."""
    first = (seq_start.view(batch, t).long() - torch.arange(batch, device=seq_start.device).view(batch, 1) * t).unsqueeze(-1)  # [B, T, 1], in-row
    j = torch.arange(t, device=seq_start.device).view(1, 1, t)
    i = torch.arange(t, device=seq_start.device).view(1, t, 1)
    return ((j <= i) & (j >= first)).unsqueeze(1)


def _mask_passthrough(batch_size=None, q_length=None, kv_length=None, q_offset=0, kv_offset=0, mask_function=None, attention_mask=None, **kwargs):
    """The mask function of "prl_varlen": the 2-D attention_mask as it came.  No 4-D mask, no `.all()`, no device sync."""
    return attention_mask


def prl_varlen_attention_forward(module, query, key, value, attention_mask=None, dropout: float = 0.0, scaling: float | None = None,
                                 is_causal: bool | None = None, sliding_window: int | None = None, softcap: float | None = None, **kwargs):
    """The function registered as "prl_varlen": `query [B, Hq, T, D]`, `key` / `value [B, Hkv, T, D]`, the 2-D attention_mask
    (or None) and `position_ids` in kwargs -> `([B, T, Hq, D], None)`."""
    batch, hq, t, d = query.shape
    if key.shape[2] != t:
        raise NotImplementedError(
            f"prl_varlen attention got {t} queries for {key.shape[2]} keys (a KV cache): install_fused_attention is for the learner's full-sequence "
            "forward; call uninstall_fused_attention(model) before generating with this model")
    if attention_mask is not None and attention_mask.dim() != 2:
        raise NotImplementedError(f"prl_varlen attention takes the 2-D attention_mask, not one of shape {tuple(attention_mask.shape)}")
    position_ids = kwargs.get("position_ids")
    if position_ids is not None and position_ids.dim() != 2:
        position_ids = None  # (multi-axis rotary positions say nothing about packing)
    if scaling is None:
        scaling = d ** -0.5
    group = getattr(module, "_prl_seq_parallel_group", None)
    if group is not None:
        return _sp_attention_forward(module, group, query, key, value, attention_mask, position_ids, dropout, scaling, sliding_window, softcap, kwargs)
    seq_start, seq_end = _cached_segments(position_ids, attention_mask, (batch, t))
    position_bias = kwargs.get("position_bias")
    kernel = (query.is_cuda and query.dtype == torch.bfloat16 and key.dtype == torch.bfloat16 and value.dtype == torch.bfloat16 and d in HEAD_SIZES
              and not dropout and sliding_window is None and softcap is None and position_bias is None and hq % key.shape[1] == 0)
    if kernel:
        n = batch * t
        # [B, H, T, D] views of token-major memory flatten without a copy; any other layout is copied once, in [B, T, H, D] order
        qf = query.transpose(1, 2).reshape(n, hq, d)
        kf = key.transpose(1, 2).reshape(n, key.shape[1], d)
        vf = value.transpose(1, 2).reshape(n, value.shape[1], d)
        out = varlen_attention(qf, kf, vf, seq_start, seq_end, scaling)
        return out.view(batch, t, hq, d), None
    from transformers.integrations.sdpa_attention import sdpa_attention_forward

    mask = block_diagonal_mask(seq_start.to(query.device), batch, t)
    if sliding_window is not None:
        i = torch.arange(t, device=query.device).view(t, 1)
        j = torch.arange(t, device=query.device).view(1, t)
        mask = mask & (i - j < sliding_window)
    extra = {k_: v_ for k_, v_ in kwargs.items() if k_ != "position_ids"}
    if softcap is not None:
        extra["softcap"] = softcap
    return sdpa_attention_forward(module, query, key, value, mask, dropout=dropout, scaling=scaling, is_causal=False, **extra)


def _register() -> None:
    from transformers import AttentionInterface
    from transformers.masking_utils import AttentionMaskInterface

    if NAME not in AttentionInterface._global_mapping:
        AttentionInterface.register(NAME, prl_varlen_attention_forward)
    if NAME not in AttentionMaskInterface._global_mapping:
        AttentionMaskInterface.register(NAME, _mask_passthrough)


def _attention_layers(lm: Any) -> tuple[int, list]:
    """(layers the kernels take, [(name, why)] of those that go to the fallback) by what the module and its config say."""
    n, skipped = 0, []
    for name, mod in lm.named_modules():
        if not (hasattr(mod, "q_proj") and hasattr(mod, "k_proj") and hasattr(mod, "v_proj")):
            continue
        d = getattr(mod, "head_dim", None)
        why = None
        if d not in HEAD_SIZES:
            why = f"head_dim {d}: the kernels are built for {HEAD_SIZES}"
        elif getattr(mod, "sliding_window", None) is not None:
            why = f"sliding_window {mod.sliding_window}"
        elif getattr(mod, "attention_dropout", 0.0):
            why = f"attention_dropout {mod.attention_dropout} (fallback while training)"
        if why is None:
            n += 1
        else:
            skipped.append((name, why + ": sdpa under the block-diagonal mask"))
    return n, skipped


def _attention_modules(lm: Any) -> list:
    return [mod for _, mod in lm.named_modules() if hasattr(mod, "q_proj") and hasattr(mod, "k_proj") and hasattr(mod, "v_proj")]


def install_fused_attention(model: Any, seq_parallel_group: Any = None) -> Any:
    """Switch a Hugging Face causal LM (bare or inside the actor-critic wrapper) to the "prl_varlen" attention: packed sequences
    (`position_ids` resets) and pad tokens (zeros of the 2-D `attention_mask`) are kept apart, through the HIP kernels for bf16
    tensors on a HIP device with head size 64 / 128, through sdpa under the equivalent block-diagonal mask otherwise.
    Registers the name with transformers once per process; only THIS model's `config._attn_implementation` changes, no module
    or parameter is touched, and `install_fused_head` / `install_fused_body` compose in any order.  The report is
    `model._prl_fused_attention = {"previous": <old name>, "layers": n, "skipped": [(name, why), ...]}`; calling it again
    changes nothing.  With a KV cache the attention raises NotImplementedError: `uninstall_fused_attention` first.

    `seq_parallel_group`: a process group of size P > 1 whose ranks each hold one `make_slices(P)` slice of a packed row (what the
    reference gets from `substitute_hf_flash_attn(group)` + `update_ring_flash_attn_params(seq_boundaries, group)` before every
    micro-batch; here the binding is made once and the gathered `position_ids` carry the boundaries).  Every attention layer then
    all-gathers K / V over the group, attends its slice's queries to the whole row and exchanges the fp32 dK / dV partials in
    backward (`seq_parallel_attention`); the report gains `"seq_parallel": P`.  A group of size 1 is the same as None.  Every
    rank of the group must run the same forwards and backwards: the collectives are part of them."""
    from .fused_head import _lm_of

    p = _group_size(seq_parallel_group)
    group = seq_parallel_group if p > 1 else None
    if getattr(model, "_prl_fused_attention", None) is not None:
        if model._prl_fused_attention.get("seq_parallel", 1) != p or (group is not None and any(
                getattr(m, "_prl_seq_parallel_group", None) is not group for m in _attention_modules(_lm_of(model)))):
            raise ValueError("install_fused_attention: this model is already installed with another sequence-parallel binding; "
                             "uninstall_fused_attention(model) first")
        return model
    lm = _lm_of(model)
    report = getattr(lm, "_prl_fused_attention", None)  # installed through another handle on the same LM
    if report is None:
        _register()
        previous = getattr(lm.config, "_attn_implementation", None)
        lm.set_attn_implementation(NAME)
        layers, skipped = _attention_layers(lm)
        report = {"previous": previous, "layers": layers, "skipped": skipped}
        if group is not None:
            report["seq_parallel"] = p
            for mod in _attention_modules(lm):
                mod._prl_seq_parallel_group = group
        lm._prl_fused_attention = report
    elif report.get("seq_parallel", 1) != p:
        raise ValueError("install_fused_attention: the language model is already installed with another sequence-parallel binding; "
                         "uninstall_fused_attention(model) first")
    model._prl_fused_attention = report
    return model


def require_seq_parallel_attention(model: Any, seq_parallel_group: Any) -> None:
    """Raise unless every attention layer of `model` is bound to `seq_parallel_group` (`install_fused_attention(model,
    seq_parallel_group=group)`).  A learner rank that is handed one slice of a packed row and runs unbound attention on it attends
    the slice alone: tokens of a sequence that began on an earlier rank never see its earlier keys, and the loss path then reduces
    wrong log-probs faithfully.  A group of size 1 (or None) and a model without attention layers pass."""
    if _group_size(seq_parallel_group) <= 1 or not hasattr(model, "modules"):
        return
    unbound = [type(m).__name__ for m in model.modules() if hasattr(m, "q_proj") and hasattr(m, "k_proj") and hasattr(m, "v_proj")
               and getattr(m, "_prl_seq_parallel_group", None) is not seq_parallel_group]
    if unbound:
        raise RuntimeError(f"{len(unbound)} attention layer(s) ({unbound[0]}, ...) are not bound to the sequence-parallel group: each rank would attend "
                           "its slice alone; call install_fused_attention(model, seq_parallel_group=group) before building the learner step")


def uninstall_fused_attention(model: Any) -> Any:
    """Back to the attention implementation the model had before `install_fused_attention`."""
    from .fused_head import _lm_of

    lm = _lm_of(model)
    report = getattr(lm, "_prl_fused_attention", None) or getattr(model, "_prl_fused_attention", None)
    if report is None:
        return model
    lm.set_attn_implementation(report["previous"] or "sdpa")
    for mod in _attention_modules(lm):  # the sequence-parallel binding goes with it
        if hasattr(mod, "_prl_seq_parallel_group"):
            del mod._prl_seq_parallel_group
    for owner in (model, lm):
        if getattr(owner, "_prl_fused_attention", None) is not None:
            del owner._prl_fused_attention
    return model
