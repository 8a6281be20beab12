"""Packed variable-length causal attention for the learner body (csrc/prl_attention.hip).

The learner hands the stock transformers body a packed `[1, T]` micro-batch with `attention_mask = ones` and per-sequence
`position_ids`.  Under `attn_implementation="sdpa"` that batch is attended as ONE sequence of T tokens: the tokens of a later
sequence see every earlier one.  The reference keeps packed sequences apart with flash-attn's varlen path, driven by the
`position_ids` resets.  This module is that path:

    segments(position_ids, attention_mask)           the two int32 arrays seq_start / seq_end over the flattened B T tokens
    varlen_attention(q, k, v, seq_start, seq_end, scale)   key j visible to query i iff seq_start[i] <= j <= i; bf16, HIP
    install_fused_attention(model)                   registers "prl_varlen" with transformers' AttentionInterface and
                                                     switches this model to it; opt-in, per model

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
    seq_start, seq_end = _cached_segments(position_ids, attention_mask, (batch, t))
    if scaling is None:
        scaling = d ** -0.5
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


def install_fused_attention(model: Any) -> Any:
    """Switch a Hugging Face causal LM (bare or inside the actor-critic wrapper) to the "prl_varlen" attention: packed sequences
    (`position_ids` resets) and pad tokens (zeros of the 2-D `attention_mask`) are kept apart, through the HIP kernels for bf16
    tensors on a HIP device with head size 64 / 128, through sdpa under the equivalent block-diagonal mask otherwise.
    Registers the name with transformers once per process; only THIS model's `config._attn_implementation` changes, no module
    or parameter is touched, and `install_fused_head` / `install_fused_body` compose in any order.  The report is
    `model._prl_fused_attention = {"previous": <old name>, "layers": n, "skipped": [(name, why), ...]}`; calling it again
    changes nothing.  With a KV cache the attention raises NotImplementedError: `uninstall_fused_attention` first."""
    from .fused_head import _lm_of

    if getattr(model, "_prl_fused_attention", None) is not None:
        return model
    lm = _lm_of(model)
    report = getattr(lm, "_prl_fused_attention", None)  # installed through another handle on the same LM
    if report is None:
        _register()
        previous = getattr(lm.config, "_attn_implementation", None)
        lm.set_attn_implementation(NAME)
        layers, skipped = _attention_layers(lm)
        report = {"previous": previous, "layers": layers, "skipped": skipped}
        lm._prl_fused_attention = report
    model._prl_fused_attention = report
    return model


def uninstall_fused_attention(model: Any) -> Any:
    """Back to the attention implementation the model had before `install_fused_attention`."""
    from .fused_head import _lm_of

    lm = _lm_of(model)
    report = getattr(lm, "_prl_fused_attention", None) or getattr(model, "_prl_fused_attention", None)
    if report is None:
        return model
    lm.set_attn_implementation(report["previous"] or "sdpa")
    for owner in (model, lm):
        if getattr(owner, "_prl_fused_attention", None) is not None:
            del owner._prl_fused_attention
    return model
