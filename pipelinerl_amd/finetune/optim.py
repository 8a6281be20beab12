"""Optimizers of the learner step: the reference's `get_grouped_params` / `get_optimizer` (pipelinerl/finetune/optim.py:8-45)
on top of fused HIP steps (csrc/prl_optim.hip).

`FusedAdamW` / `FusedLion` replace `torch.optim.AdamW` / the reference's `Lion` (:48-112) and the gradient clipping in front
of them: `clip_and_step(max_norm)` is `torch.nn.utils.clip_grad_norm_` + `step()` as one read pass over the gradients and one
read-modify-write pass over parameters and state, the clip coefficient never leaving the device (no host synchronisation
between the two, the gradients are not rewritten).  The per-element arithmetic is torch's / the reference's, operation by
operation (csrc/prl_optim_math.h).

Master weights: a bf16 parameter gets an fp32 copy in the optimizer state (`state[p]["master"]`); the update is applied to the
copy and the parameter is its round-to-nearest-even image, written where the parameter lives (so a parameter re-homed into an
exported IPC bucket is published without a copy).  Without them an update of 1e-6 on a bf16 weight of magnitude > 2.6e-4 is
below half an ulp and is rounded away - the reference relies on DeepSpeed's fp32 master weights for the same reason.

The master copy is seeded from the parameter when its state is created and is the truth from then on: whoever overwrites a
parameter afterwards (a checkpoint loaded into the model but not into the optimizer, a received weight broadcast) must also
write `state[p]["master"]` (or drop the state), otherwise the next step writes the image of the stale master back.  Moving a
parameter's storage (`ColocatedSender.rehome`) is fine: the values travel, and the new address is picked up.

Data parallelism: gradients are already reduced when the accumulation boundary is reached (DDP averages them in backward), so
the norm computed here is complete on every rank.

Sharded state (ZeRO-1; `shard_group=` a torch.distributed group, or `shard=(rank, world)` without one): the parameters, in
`param_groups` order and each padded to a 16-element slot, form one element space that is cut into `world` equal ranges of
`shard_len` elements (a multiple of 16): `plan_shards`.  A rank allocates `exp_avg`, `exp_avg_sq`, `master` and `step` for its
range only (three flat buffers of `shard_len` floats) and steps the pieces of the parameters inside it - ordinary segments of the
same kernels whose pointers are offset by a multiple of 16 elements, so the 16-byte vector path is kept.  The method names and
their order at the boundary do not change; the collectives happen inside them:
  * `grad_accum_dtype=None`: `p.grad` is complete on every rank (DDP), the norm is the unsharded one; only the step is restricted.
  * `grad_accum_dtype=torch.float32`: every parameter (fp32 ones too) has a slot in a flat accumulator laid out like the element
    space; `reduce_accumulated` reduces it to the owners (`reduce_scatter_tensor` over RCCL, `all_reduce` over gloo - the choice
    follows the backend only) and divides the own range by the world size.  No rank then holds every reduced gradient:
    `compute_grad_norm` sums the squares of the own pieces (`prl_optim_grad_sumsq`), adds the ranks' fp64 values with one
    `all_reduce`, and forms norm and coefficient from the total on the device (`prl_optim_clip_from_sumsq`).
  * `step()` updates the own pieces where the parameters live, packs them into a send buffer (`prl_bucket_gather`; the parameter's
    own dtype, 16-byte aligned pieces, padded to the largest rank's size), exchanges the buffers (`all_gather_into_tensor` /
    `all_gather`) and writes the other ranks' pieces into the parameters (`prl_bucket_scatter`).  Buffers are allocated once.
With `shard=` there is no group to call: the caller moves the data between the halves that the methods above are made of
(`prepare_reduce` / `finish_reduce`, `local_grad_sumsq` / `norm_from_sumsq`, `pack_shard` / `unpack_shards`) - one process can
stand in for every rank.  `state_dict()` is this rank's shard plus the partition; `full_state_dict()` gathers an unsharded
dictionary on rank 0, and an unsharded dictionary loads into shards (each rank takes its ranges).

Sharded gradients (ZeRO-2; `shard_grads=True` on top of sharded state with `grad_accum_dtype=torch.float32`): the flat accumulator
above is `world x shard_len` floats on every rank and is reduced once per step.  With the option a rank keeps the accumulator of its
own range only (`shard_len` floats, views for the owned pieces) and every micro-batch's gradients travel to their owners at once, in
bounded buckets: bucket k is elements `[k B, min((k + 1) B, shard_len))` of EVERY rank's range (`bucket_elems`, `plan_buckets`; B a
multiple of 16 elements such that one destination's pieces of one bucket - each in its gradient's own dtype at a 16-byte aligned
offset, a "slot" - never exceed `exchange_bucket_bytes`).  `accumulate_grads()` becomes a COLLECTIVE: per bucket it gathers this
micro-batch's pieces into a send buffer of `world` slots (`prl_bucket_gather`; a parameter without a gradient here travels as +0.0),
exchanges slot d with rank d (`all_to_all_single`, RCCL and gloo alike) and folds the `world` received copies of the own pieces into the
accumulator in rank order in one pass (`prl_optim_grad_accumulate_ranks`).  `reduce_accumulated()` then moves nothing: it divides the
own range by the world size.  The weight exchange after the step runs bucket by bucket through the same two buffers (`world x slot`
bytes each, allocated once) instead of a whole-model receive buffer; the bytes that arrive are the same.  Per rank and micro-batch
`(world - 1) / world` of the gradient bytes are sent - `world`-fold the traffic of one reduction per step when there are `world`
micro-batches, the price of the memory.  Everything is stream-ordered on the current stream and single-buffered; overlapping a bucket's
exchange with the next one's gather is not built.  With `shard=` the halves are `n_grad_buckets`, `pack_grad_bucket`,
`fold_grad_bucket`, `finish_grad_fold` and `pack_shard_bucket` / `unpack_shard_bucket`.

Gradient accumulation (`grad_accum_dtype=torch.float32`): autograd sums the micro-batch gradients into `p.grad` in the
parameter's dtype, and a bf16 running sum drops every term below half an ulp of it - after 256 equal terms all of the next one.
The reference accumulates in fp32 (FSDP `param_dtype / reduce_dtype: fp32`, DeepSpeed's fp32 gradient partitions).  With the
option, `accumulate_grads()` after every `backward()` folds each bf16 `p.grad` into an fp32 accumulator (one IEEE add per
element and micro-batch, `prl_optim_grad_accumulate`) and clears `p.grad`; norm and step read the accumulators;
`reduce_accumulated(group)` averages them over the data-parallel ranks in fp32 (run every pass under `no_sync()`: DDP would
reduce the last micro-batch's `p.grad` only).  fp32 gradients (the fp32 `lm_head`, which the fused head already accumulates
into in fp32) are used as they are.  The accumulators are views of one flat buffer, transient (not in `state_dict()`), and
cost 4 bytes per bf16 element: 28 GB on the Qwen2.5-7B list.

Compact state (`state_dtype=torch.bfloat16`, `param_rounding="stochastic"`, `seed=`; `FusedAdamW` / `FusedLion`, csrc/prl_optim_compact.hip):
`exp_avg` / `exp_avg_sq` are kept in bf16 - widened exactly on load, the fp32 update unchanged, the store rounded STOCHASTICALLY - and a
bf16 parameter without a master copy (`master_weights=False`) is written with stochastic rounding, so that an update below half an ulp
survives in expectation instead of being rounded away (round-to-nearest cannot even decay a bf16 second moment: 0.999 v rounds back
to v).  State per bf16 element: AdamW 12 -> 4 bytes, Lion 8 -> 2.  The two options are independent; `param_rounding="stochastic"` has
no effect on a parameter that has a master copy (the master stays the truth and the parameter its nearest image) or is fp32 (written
exactly).  The random bits are a pure function of (seed, parameter's index in `param_groups` order, element's index inside the
parameter, step): Philox4x32-10, csrc/prl_optim_sr.h.  Hence a sharded run produces the bits of the unsharded one, two runs with one
seed agree, and a run resumed from `state_dict()` (which carries `seed` in `param_groups` and the counter in `step`) continues bit for
bit.  `state_dict()` holds the moments in `state_dtype`; `load_state_dict` converts a loaded moment to this optimizer's `state_dtype`
(bf16 -> fp32 exactly; fp32 -> bf16 to nearest even, once).  The defaults (`torch.float32`, `"nearest"`) run the kernels and entry
points above, untouched.

`FusedAdafactor` (`get_optimizer("adafactor_hip")`) is transformers' Adafactor with the reference's flags on the same host side
(csrc/prl_adafactor.hip): the same boundary protocol, master weights and fp32 accumulation; factored state under transformers'
keys; no sharded state.

There is no CPU path: parameters that are not on a HIP device raise.
"""

from __future__ import annotations

import ctypes
from typing import Any, Iterable

import torch

from .. import _lib

_DTYPES = {torch.float32: _lib.PRL_DTYPE_F32, torch.bfloat16: _lib.PRL_DTYPE_BF16}
_SLOT = 16  # state slots are padded to 16 elements so that every view of the flat buffers is 64-byte aligned


def get_grouped_params(model: torch.nn.Module, weight_decay: float, no_decay: list[str] = ["bias", "LayerNorm.weight"]):
    """The reference's grouping rule and return shape: two groups in `named_parameters()` order, the first with `weight_decay`,
    the second (every parameter whose name contains one of the `no_decay` substrings) with 0."""
    groups: tuple[list, list] = ([], [])
    for name, param in model.named_parameters():
        exempt = any(fragment in name for fragment in no_decay)
        groups[int(exempt)].append(param)
    return [{"params": groups[0], "weight_decay": weight_decay}, {"params": groups[1], "weight_decay": 0.0}]


def shard_layout(numels, world: int, slot: int = _SLOT) -> tuple[list[int], int]:
    """(offset of every parameter in the slot-padded element space, shard_len): the padded length rounded up to `world` ranges of
    a multiple of `slot` elements."""
    if world < 1 or slot < 1:
        raise ValueError(f"plan_shards: world ({world}) and slot ({slot}) must be positive")
    offsets, off = [], 0
    for n in numels:
        offsets.append(off)
        off += -(-int(n) // slot) * slot
    return offsets, -(-off // (world * slot)) * slot


def plan_shards(numels, world: int, slot: int = _SLOT) -> list[list[tuple[int, int, int]]]:
    """The partition of sharded optimizer state: per rank the list of `(param_index, begin, end)` element ranges it owns.
    Rank r owns `[r shard_len, (r + 1) shard_len)` of the padded space, so every `begin` is a multiple of `slot` inside its
    parameter and only a piece's length can be ragged.  A world larger than the slot count leaves the last ranks empty."""
    offsets, shard_len = shard_layout(numels, world, slot)
    plan = []
    for r in range(world):
        lo, hi = r * shard_len, (r + 1) * shard_len
        pieces = []
        for i, (off, n) in enumerate(zip(offsets, numels)):
            b, e = max(off, lo) - off, min(off + int(n), hi) - off
            if e > b:
                pieces.append((i, b, e))
        plan.append(pieces)
    return plan


def bucket_elems(exchange_bucket_bytes: int, widest: int = 4, slot: int = _SLOT) -> int:
    """B of the bucketed exchange: the largest multiple of `slot` elements whose pieces fit `exchange_bucket_bytes` when every element
    is `widest` bytes.  (Pieces begin on slot boundaries of the element space and a slot of elements is a multiple of 16 bytes, so the
    16-byte padding of the pieces of one bucket stays inside `B x widest` bytes.)"""
    if isinstance(exchange_bucket_bytes, bool) or not isinstance(exchange_bucket_bytes, int) or exchange_bucket_bytes < slot * 4:
        raise ValueError(f"fused optimizer: exchange_bucket_bytes must be an int of at least {slot * 4} bytes (one slot of fp32 elements), got {exchange_bucket_bytes!r}")
    return exchange_bucket_bytes // (slot * widest) * slot


def plan_buckets(numels, itemsizes, world: int, bucket: int, slot: int = _SLOT):
    """The bucketed exchange of sharded gradients / weights: `(n_buckets, slot_bytes, pieces)`.  Bucket k covers elements
    `[k bucket, min((k + 1) bucket, shard_len))` of every rank's range of the padded element space (`shard_layout`);
    `pieces[k][d]` lists what of it belongs to rank d as `(param_index, begin, end, byte_offset)`: element range inside the parameter
    and where the piece stands in the slot - pieces in order, each at a 16-byte aligned offset, `itemsizes[param_index]` bytes per
    element (the layout rule of the whole-buffer weight exchange).  `slot_bytes` is the largest slot, at least 16."""
    if bucket < slot or bucket % slot:
        raise ValueError(f"plan_buckets: bucket ({bucket}) must be a positive multiple of the slot ({slot})")
    offsets, shard_len = shard_layout(numels, world, slot)
    n_buckets = max(1, -(-shard_len // bucket))
    pieces = [[[] for _ in range(world)] for _ in range(n_buckets)]
    slot_bytes = 16
    for d in range(world):
        i = 0
        for k in range(n_buckets):
            lo, hi = d * shard_len + k * bucket, d * shard_len + min((k + 1) * bucket, shard_len)
            while i < len(numels) and offsets[i] + int(numels[i]) <= lo:
                i += 1
            j, at = i, 0
            while j < len(numels) and offsets[j] < hi:
                b, e = max(offsets[j], lo) - offsets[j], min(offsets[j] + int(numels[j]), hi) - offsets[j]
                if e > b:
                    pieces[k][d].append((j, b, e, at))
                    at += -(-(e - b) * itemsizes[j] // 16) * 16
                j += 1
            slot_bytes = max(slot_bytes, at)
    return n_buckets, slot_bytes, pieces


def _resolve_shard(shard_group, shard) -> tuple[int, int] | None:
    """(rank, world) of the sharded state, None for a world of one (today's unsharded behaviour)."""
    if shard_group is not None and shard is not None:
        raise ValueError("fused optimizer: give shard_group= (a torch.distributed group) or shard=(rank, world), not both")
    if shard is not None:
        rank, world = int(shard[0]), int(shard[1])
        if world < 1 or not 0 <= rank < world:
            raise ValueError(f"fused optimizer: shard=(rank, world): rank {rank} is not in [0, {world})")
    elif shard_group is not None:
        import torch.distributed as dist

        rank, world = dist.get_rank(shard_group), dist.get_world_size(shard_group)
    else:
        return None
    return (rank, world) if world > 1 else None


def merge_shard_state_dicts(shards: list[dict]) -> dict:
    """The unsharded state dictionary of the `state_dict()`s of every rank of one sharded optimizer."""
    shards = sorted(shards, key=lambda d: d["shard"]["rank"])
    meta = shards[0]["shard"]
    if [d["shard"]["rank"] for d in shards] != list(range(meta["world"])):
        raise ValueError(f"merge_shard_state_dicts: need the shard of every rank of a world of {meta['world']}, got ranks {[d['shard']['rank'] for d in shards]}")
    state: dict[int, dict] = {}
    for d in shards:
        for pid, st in d["state"].items():
            b, e = d["shard"]["ranges"][pid]
            full = state.setdefault(pid, {})
            for k, v in st.items():
                if k == "step":
                    full[k] = torch.as_tensor(v, dtype=torch.float32).detach().cpu().clone()
                    continue
                if k not in full:
                    full[k] = torch.zeros(meta["numels"][pid], dtype=v.dtype, device=v.device)
                full[k][b:e] = v.reshape(-1)
    for pid, st in state.items():
        for k in st:
            if k != "step":
                st[k] = st[k].view(meta["shapes"][pid])
    import copy

    return {"state": state, "param_groups": copy.deepcopy(shards[0]["param_groups"])}


def _check_hyper(lr: float, betas: tuple[float, float], weight_decay: float, eps: float = 0.0) -> None:
    if not 0.0 <= lr:
        raise ValueError(f"Invalid learning rate: {lr}")
    if not 0.0 <= eps:
        raise ValueError(f"Invalid epsilon value: {eps}")
    if not 0.0 <= betas[0] < 1.0:
        raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
    if not 0.0 <= betas[1] < 1.0:
        raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
    if not 0.0 <= weight_decay:
        raise ValueError(f"Invalid weight_decay value: {weight_decay}")


_ROUNDINGS = {"nearest": _lib.PRL_ROUND_NEAREST, "stochastic": _lib.PRL_ROUND_STOCHASTIC}


def _check_compact(state_dtype, param_rounding, seed) -> torch.dtype:
    """Validates the compact-state options; returns the dtype of the moments (None means fp32)."""
    state_dtype = torch.float32 if state_dtype is None else state_dtype
    if state_dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"fused optimizer: state_dtype must be torch.float32 or torch.bfloat16 (got {state_dtype})")
    if param_rounding not in _ROUNDINGS:
        raise ValueError(f'fused optimizer: param_rounding must be "nearest" or "stochastic" (got {param_rounding!r})')
    if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 1 << 64:
        raise ValueError(f"fused optimizer: seed must be an int in [0, 2^64) (got {seed!r})")
    return state_dtype


class _FusedOptimizer(torch.optim.Optimizer):
    """Shared host side of the fused steps: lazily allocated flat state (fp32, or bf16 moments), the segment table, the norm record."""

    _state_keys: tuple[str, ...] = ("exp_avg",)
    _segment_type = _lib.PrlOptimSegment  # what `_launch` hands to `_call`

    def __init__(self, params: Iterable, defaults: dict[str, Any], master_weights: bool, grad_accum_dtype: torch.dtype | None = None,
                 shard_group=None, shard: tuple[int, int] | None = None, state_dtype: torch.dtype | None = None, param_rounding: str = "nearest",
                 shard_grads: bool = False, exchange_bucket_bytes: int = 64 << 20):
        if grad_accum_dtype not in (None, torch.float32):
            raise ValueError(f"fused optimizer: grad_accum_dtype must be None or torch.float32 (got {grad_accum_dtype})")
        bucket_elems(exchange_bucket_bytes)  # (raises below one slot)
        if shard_grads and grad_accum_dtype != torch.float32:
            raise ValueError("fused optimizer: shard_grads=True shards the fp32 gradient accumulators: it needs grad_accum_dtype=torch.float32")
        if shard_grads and shard_group is None and shard is None:
            raise ValueError("fused optimizer: shard_grads=True needs sharded state (shard_group= or shard=)")
        self.state_dtype = _check_compact(state_dtype, param_rounding, defaults.get("seed", 0))
        self.param_rounding = param_rounding
        self._compact = self.state_dtype != torch.float32 or param_rounding != "nearest"  # the step goes through the compact entry points
        self._compact_table = None                # ctypes array of PrlOptimCompactSegment, entry for entry next to `_table`
        if self._compact:
            self._segment_type = _lib.PrlOptimCompactSegment
        self._shard = _resolve_shard(shard_group, shard)  # (rank, world), world > 1; None: unsharded
        self._shard_group = shard_group if self._shard is not None else None
        self.shard_grads = bool(shard_grads) and self._shard is not None  # (a world of one: today's unsharded behaviour)
        self.exchange_bucket_bytes = exchange_bucket_bytes
        self._gx = None                           # sharded gradients: the bucket plan and the two exchange buffers
        self._folded = False                      # sharded gradients: a micro-batch was folded since the last step / zero_grad
        super().__init__(params, defaults)
        self._lay = None                          # sharded: (numels, params, offsets, shard_len, {param index: (begin, end)})
        self._shard_flat: dict[str, torch.Tensor] = {}  # sharded: state key -> flat buffer of shard_len floats
        self._reduced = False                     # sharded fp32 accumulation: the own range holds the averaged gradients
        self._sumsq: torch.Tensor | None = None   # sharded: device fp64, the sum of squares of the own pieces
        self._norm_table = None                   # sharded, complete p.grad: every gradient whole, for the norm
        self._pub = None                          # sharded: send / receive buffers and the piece layout of the weight exchange
        self._pub_tables = None
        self._device: torch.device | None = None
        self.master_weights = bool(master_weights)
        self.grad_accum_dtype = grad_accum_dtype
        self._acc_flat: torch.Tensor | None = None      # the flat fp32 accumulator buffer (slot-padded like the state)
        self._acc: dict[torch.Tensor, torch.Tensor] = {}  # parameter -> its view of the buffer
        self._acc_filled: set[torch.Tensor] = set()     # folded at least once since the last step / zero_grad
        self._acc_zeroed: dict[torch.Tensor, tuple[torch.Tensor, int]] = {}  # accumulate_grads(set_to_none=False): the zeroed p.grad and its version
        self._flat: list[torch.Tensor] = []       # the flat state buffers (kept alive here; state entries are views)
        self._table = None                        # ctypes array of PrlOptimSegment, one per parameter
        self._table_key: list[tuple[int, int]] = []
        self._table_params: list[tuple[torch.Tensor, dict]] = []
        self._workspace: torch.Tensor | None = None
        self._record: torch.Tensor | None = None  # device: [total_norm, clip_coef]

    # ---- state ----------------------------------------------------------------------------------------------------------
    def _wants_master(self, p: torch.Tensor) -> bool:
        return self.master_weights and p.dtype != torch.float32

    def _keys_of(self, p: torch.Tensor) -> tuple[str, ...]:
        return self._state_keys + (("master",) if self._wants_master(p) else ())

    def _dtype_of(self, key: str) -> torch.dtype:
        """dtype of `state[p][key]`: `state_dtype` for the moments, fp32 for the master copy."""
        return torch.float32 if key == "master" else self.state_dtype

    def _state_shape(self, p: torch.Tensor, key: str) -> torch.Size:
        """Shape of `state[p][key]`: the parameter's, unless the rule keeps less (Adafactor's row / column averages)."""
        return p.shape

    def _is_flat_view(self, t: torch.Tensor) -> bool:
        return any(t.untyped_storage().data_ptr() == f.untyped_storage().data_ptr() for f in self._flat)

    def _ensure_state(self) -> None:
        """State of every parameter that has a gradient and none yet (or a loaded one that is not in a flat buffer)."""
        if self._shard is not None:
            return self._ensure_state_sharded()
        for group in self.param_groups:
            todo = []
            for p in group["params"]:
                if self._grad_of(p) is None:
                    continue
                st = self.state[p]
                keys = self._keys_of(p)
                if all(k in st and st[k].dtype == self._dtype_of(k) and st[k].device == p.device and self._is_flat_view(st[k]) for k in keys) and "step" in st:
                    continue
                todo.append(p)
            if not todo:
                continue
            device = todo[0].device
            for key in self._state_keys + ("master",):
                owners = [p for p in todo if key in self._keys_of(p)]
                if not owners:
                    continue
                shapes = [self._state_shape(p, key) for p in owners]
                slots = [(-(-shape.numel() // _SLOT)) * _SLOT for shape in shapes]
                flat = torch.zeros(sum(slots), dtype=self._dtype_of(key), device=device)
                self._flat.append(flat)
                off = 0
                for p, slot, shape in zip(owners, slots, shapes):
                    view = flat[off:off + shape.numel()].view(shape)
                    off += slot
                    st = self.state[p]
                    if key in st:  # loaded from a checkpoint: keep its values
                        view.copy_(st[key].to(device=device, dtype=flat.dtype).reshape(shape))
                    elif key == "master":
                        view.copy_(p.detach())
                    st[key] = view
            for p in todo:
                self.state[p].setdefault("step", torch.tensor(0.0, dtype=torch.float32))
        self._flat = [f for f in self._flat if any(self._owns(f, st) for st in self.state.values())]

    # ---- sharded state --------------------------------------------------------------------------------------------------
    def _layout(self):
        params = [p for group in self.param_groups for p in group["params"]]
        numels = tuple(p.numel() for p in params)
        if self._lay is None or self._lay[0] != numels:
            if self._lay is not None and (self._shard_flat or self._acc_flat is not None):
                raise RuntimeError("fused optimizer: the parameter list changed after the sharded state was allocated; the partition is fixed by then")
            rank, world = self._shard
            offsets, shard_len = shard_layout(numels, world)
            mine = {i: (b, e) for i, b, e in plan_shards(numels, world)[rank]}
            if rank == 0:  # a parameter without elements has no piece; its step count lives on rank 0, so that the gathered state is complete
                mine.update({i: (0, 0) for i, n in enumerate(numels) if n == 0})
            self._lay = (numels, params, offsets, shard_len, mine)
            self._pub = self._pub_tables = self._gx = None
        return self._lay

    @property
    def shard_len(self) -> int | None:
        """Elements of the padded parameter space this rank owns (None: unsharded)."""
        return None if self._shard is None else self._layout()[3]

    def _ensure_state_sharded(self) -> None:
        """The flat buffers hold this rank's range only; an owned piece gets its views once its parameter has a gradient."""
        _, params, offsets, shard_len, mine = self._layout()
        if not params:
            return
        device = params[0].device
        if not self._shard_flat:
            keys = self._state_keys + (("master",) if any(self._wants_master(p) for p in params) else ())
            self._shard_flat = {k: torch.zeros(shard_len, dtype=self._dtype_of(k), device=device) for k in keys}
            self._flat = list(self._shard_flat.values())
        lo = self._shard[0] * shard_len
        for i, p in enumerate(params):
            if i not in mine or self._grad_of(p) is None:
                continue
            b, e = mine[i]
            st = self.state[p]
            for k in self._keys_of(p):
                view = self._shard_flat[k][offsets[i] + b - lo:offsets[i] + e - lo]
                cur = st.get(k)
                if cur is not None and cur.data_ptr() == view.data_ptr() and cur.numel() == view.numel() and self._is_flat_view(cur):
                    continue
                if cur is not None:  # loaded from a checkpoint: keep its values
                    if cur.numel() != e - b:
                        raise ValueError(f"fused optimizer: loaded state '{k}' of parameter {i} has {cur.numel()} elements, its piece [{b}, {e}) has {e - b}")
                    view.copy_(cur.to(device=device, dtype=view.dtype).reshape(-1))
                elif k == "master":
                    view.copy_(p.detach().reshape(-1)[b:e])
                st[k] = view
            st.setdefault("step", torch.tensor(0.0, dtype=torch.float32))

    def state_dict(self) -> dict:
        """Unsharded: torch's.  Sharded: this rank's pieces (1-D) under torch's keys, plus `"shard"`: the partition."""
        d = super().state_dict()
        if self._shard is not None:
            numels, params, _, shard_len, mine = self._layout()
            d["shard"] = {"world": self._shard[1], "rank": self._shard[0], "slot": _SLOT, "total_slots": self._shard[1] * shard_len // _SLOT,
                          "shard_len": shard_len, "numels": list(numels), "shapes": [tuple(p.shape) for p in params],
                          "ranges": {i: be for i, be in mine.items()}}
        return d

    def full_state_dict(self, group=None) -> dict | None:
        """The unsharded dictionary on rank 0 of the group (None elsewhere): every rank's shard travels through the host
        (`gather_object`) - a checkpoint path, not a step path.  An unsharded optimizer loads it and continues identically.
        With `shard=` there is no group: collect every stand-in's `state_dict()` and call `merge_shard_state_dicts`."""
        d = self.state_dict()
        if self._shard is None:
            return d
        import torch.distributed as dist

        group = self._shard_group if group is None else group
        if group is None:
            raise RuntimeError("fused optimizer: full_state_dict() needs the group (shard=: use merge_shard_state_dicts on every rank's state_dict())")
        d["state"] = {pid: {k: (v.detach().cpu() if isinstance(v, torch.Tensor) else v) for k, v in st.items()} for pid, st in d["state"].items()}
        rank, world = self._shard
        gathered = [None] * world if rank == 0 else None
        dist.gather_object(d, gathered, dst=dist.get_global_rank(group, 0), group=group)
        return merge_shard_state_dicts(gathered) if rank == 0 else None

    @staticmethod
    def _owns(flat: torch.Tensor, st: dict) -> bool:
        ptr = flat.untyped_storage().data_ptr()
        return any(isinstance(v, torch.Tensor) and v.numel() and v.untyped_storage().data_ptr() == ptr for v in st.values())

    def load_state_dict(self, state_dict: dict) -> None:
        """torch casts loaded state to the parameter's dtype; the state here is fp32 (the moments: `state_dtype`) whatever the
        parameter is, so the saved tensors are taken as they are (a torch.optim.AdamW checkpoint of fp32 parameters loads: same keys)
        and converted to this optimizer's dtypes: bf16 moments widen exactly, fp32 moments go to bf16 by round-to-nearest-even, once.
        Sharded: a shard dictionary of the same world and rank, or an unsharded one from which this rank takes its ranges."""
        saved = state_dict.get("shard")
        here = self._shard or (0, 1)
        if saved is not None and (saved["rank"], saved["world"]) != here:
            raise ValueError(f"fused optimizer: this state was saved by rank {saved['rank']} of a world of {saved['world']} and cannot be loaded into "
                             f"rank {here[0]} of a world of {here[1]}; gather it with full_state_dict() and load the unsharded dictionary")
        if self._shard is not None:
            return self._load_state_dict_sharded(state_dict, saved is not None)
        super().load_state_dict(state_dict)
        saved_ids = [i for g in state_dict["param_groups"] for i in g["params"]]
        ours = [p for g in self.param_groups for p in g["params"]]
        for pid, p in zip(saved_ids, ours):
            src = state_dict["state"].get(pid)
            if src is None:
                continue
            for k in self._state_keys + ("master",):
                if k in src:
                    self.state[p][k] = src[k].detach().to(device=p.device, dtype=self._dtype_of(k)).clone()
            if "step" in src:
                self.state[p]["step"] = torch.as_tensor(src["step"], dtype=torch.float32).detach().cpu().clone()
        self._flat, self._table, self._table_key = [], None, []
        self._after_load()

    def _after_load(self) -> None:
        for group in self.param_groups:  # a dictionary saved before `seed` existed (or by torch.optim.AdamW) has none
            if "seed" in self.defaults:
                group.setdefault("seed", self.defaults["seed"])

    def _load_state_dict_sharded(self, state_dict: dict, pieces: bool) -> None:
        """Hyper-parameters through torch; of the state only the own ranges are brought to the device."""
        super().load_state_dict({"state": {}, "param_groups": state_dict["param_groups"]})
        saved_ids = [i for g in state_dict["param_groups"] for i in g["params"]]
        _, params, _, _, mine = self._layout()
        for i, (pid, p) in enumerate(zip(saved_ids, params)):
            src = state_dict["state"].get(pid)
            if src is None or i not in mine:
                continue
            b, e = mine[i]
            for k in self._state_keys + ("master",):
                if k in src:
                    t = src[k].detach().reshape(-1)
                    self.state[p][k] = (t if pieces else t[b:e]).to(device=p.device, dtype=self._dtype_of(k)).clone()
            if "step" in src:
                self.state[p]["step"] = torch.as_tensor(src["step"], dtype=torch.float32).detach().cpu().clone()
        self._shard_flat, self._flat, self._table, self._table_key = {}, [], None, []
        self._after_load()

    # ---- fp32 gradient accumulation ---------------------------------------------------------------------------------------
    def _grad_of(self, p: torch.Tensor) -> torch.Tensor | None:
        """What norm and step read for `p`: its accumulator once something was folded into it, else `p.grad`."""
        if p in self._acc_filled:
            return self._acc[p]
        return p.grad

    @staticmethod
    def _accumulates(p: torch.Tensor) -> bool:
        """The static rule (the same on every rank): a parameter whose gradient dtype is not fp32 has an accumulator."""
        return (getattr(p, "grad_dtype", None) or p.dtype) != torch.float32

    def _has_slot(self, p: torch.Tensor) -> bool:
        """Sharded: every parameter has an accumulator slot (the flat buffer is what the ranks reduce), fp32 gradients included."""
        return self._shard is not None or self._accumulates(p)

    def _unfolded(self, p: torch.Tensor) -> bool:
        g = p.grad
        if g is None or (g.dtype == torch.float32 and self._shard is None):
            return False
        z = self._acc_zeroed.get(p)
        return not (z is not None and z[0] is g and z[1] == g._version)  # zeroed in place by the last fold and untouched since

    def _check_all_folded(self) -> None:
        if self.grad_accum_dtype is None:
            return
        left = sum(self._unfolded(p) for group in self.param_groups for p in group["params"])
        if left:
            raise RuntimeError(f"fused optimizer: {left} parameter(s) hold a micro-batch gradient that was not folded into the fp32 accumulators; "
                               "call accumulate_grads() after every backward()")

    def _ensure_accumulators(self, extra: Iterable[torch.Tensor] = ()) -> None:
        """One flat fp32 buffer with a 64-byte aligned slot per accumulating parameter; rebuilt (filled slots copied) when a parameter joins."""
        if self._shard is not None:
            return self._ensure_accumulators_sharded()
        owners = [p for group in self.param_groups for p in group["params"] if self._accumulates(p) or p in self._acc]
        have = {id(p) for p in owners}
        owners += [p for p in extra if id(p) not in have]
        if self._acc_flat is not None and len(owners) == len(self._acc) and all(p in self._acc for p in owners):
            return
        if not owners:
            return
        devices = {p.device for p in owners}
        if len(devices) > 1:
            raise ValueError(f"fused optimizer: all parameters must live on one device (got {sorted(map(str, devices))})")
        slots = [(-(-p.numel() // _SLOT)) * _SLOT for p in owners]
        flat = torch.zeros(sum(slots), dtype=torch.float32, device=owners[0].device)  # zeros: the padding takes part in the all-reduce
        views, off = {}, 0
        for p, slot in zip(owners, slots):
            views[p] = flat[off:off + p.numel()].view(p.shape)
            off += slot
            if p in self._acc_filled:
                views[p].copy_(self._acc[p])
        self._acc_flat, self._acc = flat, views

    def _ensure_accumulators_sharded(self) -> None:
        """One flat fp32 buffer over the whole padded parameter space (world x shard_len): what the ranks reduce to its owners."""
        if self._acc_flat is not None:
            self._layout()  # (raises when the parameter list changed)
            return
        _, params, offsets, shard_len, mine = self._layout()
        if not params:
            return
        devices = {p.device for p in params}
        if len(devices) > 1:
            raise ValueError(f"fused optimizer: all parameters must live on one device (got {sorted(map(str, devices))})")
        if self.shard_grads:  # this rank's range only; an owned piece's view is 1-D, its elements [begin, end) of the parameter
            lo = self._shard[0] * shard_len
            flat = torch.zeros(shard_len, dtype=torch.float32, device=params[0].device)
            self._acc_flat = flat
            self._acc = {params[i]: flat[offsets[i] + b - lo:offsets[i] + e - lo] for i, (b, e) in sorted(mine.items())}
            return
        flat = torch.zeros(self._shard[1] * shard_len, dtype=torch.float32, device=params[0].device)
        self._acc_flat, self._acc = flat, {p: flat[off:off + p.numel()].view(p.shape) for p, off in zip(params, offsets)}

    @torch.no_grad()
    def accumulate_grads(self, set_to_none: bool = True) -> None:
        """Call after every micro-batch's `backward()`: folds each present non-fp32 `p.grad` into its fp32 accumulator
        (`acc = g.float()` on a parameter's first fold since the last step / `zero_grad()`, `acc += g.float()` afterwards, one fp32
        add per element) and sets `p.grad = None`, so that the next backward moves its gradient in instead of adding to a stale one
        (`set_to_none=False`: zeroed in place).  fp32 gradients are left alone: they already accumulate in fp32."""
        if self.grad_accum_dtype is None:
            raise RuntimeError("fused optimizer: accumulate_grads() needs grad_accum_dtype=torch.float32")
        if self.shard_grads:
            return self._accumulate_grads_sharded(set_to_none)
        todo = [p for group in self.param_groups for p in group["params"] if self._unfolded(p)]
        if not todo:
            return
        for p in todo:
            self._check_tensor(p, p.grad)
        self._ensure_accumulators(todo)
        lib, stream = _lib.load(), _lib.current_stream_ptr(todo[0].device)
        first = [p for p in todo if p not in self._acc_filled]
        for overwrite, part in ((1, first), (0, [p for p in todo if p in self._acc_filled])):
            if not part:
                continue
            table = (_lib.PrlAccumSegment * len(part))()  # the library cuts it into launches of 64 segments
            for seg, p in zip(table, part):
                seg.grad, seg.acc, seg.numel, seg.grad_dtype = p.grad.data_ptr(), self._acc[p].data_ptr(), p.numel(), _DTYPES[p.grad.dtype]
            _lib.check(lib.prl_optim_grad_accumulate(table, len(part), overwrite, stream))
        self._acc_filled.update(todo)
        for p in todo:
            if set_to_none:
                p.grad = None  # (freed in stream order: the fold above has been enqueued)
                self._acc_zeroed.pop(p, None)
            else:
                p.grad.zero_()
                self._acc_zeroed[p] = (p.grad, p.grad._version)

    @torch.no_grad()
    def reduce_accumulated(self, group=None) -> None:
        """Average the gradients over the data-parallel ranks in fp32: all_reduce(SUM) of the flat accumulator buffer and of every
        fp32 `p.grad` that bypasses it, divided by the group size.  A slot that is empty on this rank contributes zeros; afterwards
        every slot counts as having a gradient, so the ranks take identical steps.  RCCL reduces the device tensors; gloo stages them
        through the host inside torch.distributed.  No-op without an initialised group or with one rank."""
        import torch.distributed as dist

        if self.grad_accum_dtype is None:
            raise RuntimeError("fused optimizer: reduce_accumulated() needs grad_accum_dtype=torch.float32")
        if self.shard_grads:
            return self._reduce_sharded_grads()
        if self._shard is not None:
            return self._reduce_accumulated_sharded(group)
        if not (dist.is_available() and dist.is_initialized()):
            return
        world = dist.get_world_size(group)
        if world == 1:
            return
        self._check_all_folded()
        self._ensure_accumulators()
        for p, view in self._acc.items():
            if p not in self._acc_filled:
                view.zero_()
        if self._acc_flat is not None:
            dist.all_reduce(self._acc_flat, op=dist.ReduceOp.SUM, group=group)
            self._acc_flat.div_(world)
            self._acc_filled.update(self._acc)
        for g in self.param_groups:
            for p in g["params"]:
                if p in self._acc:
                    continue
                if p.grad is None:
                    p.grad = torch.zeros_like(p, dtype=torch.float32)
                dist.all_reduce(p.grad, op=dist.ReduceOp.SUM, group=group)
                p.grad.div_(world)

    def _reduce_accumulated_sharded(self, group=None) -> None:
        """Reduce the flat accumulator to its owners and average the own range.  RCCL: `reduce_scatter_tensor` in place (the output
        is the own range of the input, the in-place form of the collective); gloo has no reduce-scatter: `all_reduce`."""
        import torch.distributed as dist

        if self._shard_group is None:
            raise RuntimeError("fused optimizer: shard= has no group to reduce over; move the data between prepare_reduce() and finish_reduce()")
        group = self._shard_group
        if dist.get_world_size(group) != self._shard[1]:
            raise RuntimeError(f"fused optimizer: the state is sharded over {self._shard[1]} ranks, the group has {dist.get_world_size(group)}")
        flat = self.prepare_reduce()
        if dist.get_backend(group) == "nccl":
            rank, shard_len = self._shard[0], self._layout()[3]
            dist.reduce_scatter_tensor(flat[rank * shard_len:(rank + 1) * shard_len], flat, op=dist.ReduceOp.SUM, group=group)
        else:
            dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=group)
        self.finish_reduce()

    @torch.no_grad()
    def prepare_reduce(self) -> torch.Tensor:
        """Sharded fp32 accumulation, first half of `reduce_accumulated`: the flat accumulator (world x shard_len floats) with every
        slot that received nothing zeroed, ready to be summed over the ranks."""
        if self._shard is None or self.grad_accum_dtype is None:
            raise RuntimeError("fused optimizer: prepare_reduce() belongs to sharded state with grad_accum_dtype=torch.float32")
        self._no_whole_buffer("prepare_reduce() / finish_reduce()", "pack_grad_bucket(k) / fold_grad_bucket(k, received) / finish_grad_fold() after every backward")
        self._check_all_folded()
        self._ensure_accumulators()
        for p, view in self._acc.items():
            if p not in self._acc_filled:
                view.zero_()
        return self._acc_flat

    @torch.no_grad()
    def finish_reduce(self, owned: torch.Tensor | None = None) -> None:
        """Second half: `owned` = the sum over the ranks of this rank's range (None: it already stands in the accumulator); the
        range is divided by the world size and every slot counts as having a gradient, so the ranks take identical steps."""
        self._no_whole_buffer("prepare_reduce() / finish_reduce()", "pack_grad_bucket(k) / fold_grad_bucket(k, received) / finish_grad_fold() after every backward")
        rank, world = self._shard
        shard_len = self._layout()[3]
        mine = self._acc_flat[rank * shard_len:(rank + 1) * shard_len]
        if owned is not None:
            mine.copy_(owned)
        mine.div_(world)
        self._acc_filled.update(self._acc)
        self._reduced = True

    def zero_grad(self, set_to_none: bool = True) -> None:
        """Clears `p.grad` as torch does and marks every accumulator empty (no memset: the next fold overwrites)."""
        super().zero_grad(set_to_none=set_to_none)
        self._acc_filled.clear()
        self._acc_zeroed.clear()
        self._reduced = False
        self._folded = False

    # ---- sharded gradients (ZeRO-2) ------------------------------------------------------------------------------------------
    def _no_whole_buffer(self, what: str, instead: str) -> None:
        if self.shard_grads:
            raise RuntimeError(f"fused optimizer: {what} move whole buffers, which shard_grads=True does not allocate; use {instead}")

    @staticmethod
    def _grad_dtype(p: torch.Tensor) -> torch.dtype:
        """The dtype a parameter's gradient travels in: a static rule, so that a rank without the gradient lays its zeros out alike."""
        return getattr(p, "grad_dtype", None) or p.dtype

    def _exchange(self) -> dict:
        """The bucket plan (gradient pieces in the gradient's dtype, weight pieces in the parameter's; one B for both) and the two
        buffers of `world x slot` bytes that both exchanges go through.  Allocated once."""
        numels, params, offsets, shard_len, _ = self._layout()
        if self._gx is None:
            if not params:
                raise ValueError("fused optimizer: no parameters")
            devices = {p.device for p in params}
            if len(devices) > 1:
                raise ValueError(f"fused optimizer: all parameters must live on one device (got {sorted(map(str, devices))})")
            _lib.require_device(*params)
            world = self._shard[1]
            g_sizes = [torch.empty((), dtype=self._grad_dtype(p)).element_size() for p in params]
            w_sizes = [p.element_size() for p in params]
            bucket = bucket_elems(self.exchange_bucket_bytes, max(g_sizes + w_sizes))
            n, g_slot, g_pieces = plan_buckets(numels, g_sizes, world, bucket)
            _, w_slot, w_pieces = plan_buckets(numels, w_sizes, world, bucket)
            slot = max(g_slot, w_slot)
            device = params[0].device
            self._gx = {"bucket": bucket, "n": n, "slot": slot, "grad": g_pieces, "weight": w_pieces, "g_sizes": g_sizes,
                        "send": torch.zeros(world * slot, dtype=torch.uint8, device=device), "recv": torch.zeros(world * slot, dtype=torch.uint8, device=device)}
        return self._gx

    def n_grad_buckets(self) -> int:
        """Sharded gradients: the number of buckets one micro-batch's gradients (and the weights after the step) travel in."""
        if not self.shard_grads:
            raise RuntimeError("fused optimizer: n_grad_buckets() belongs to shard_grads=True")
        return self._exchange()["n"]

    @torch.no_grad()
    def pack_grad_bucket(self, k: int) -> torch.Tensor:
        """Sharded gradients, first half of a bucket's fold: this rank's send buffer for bucket `k` (uint8, `world` slots; slot d holds
        this micro-batch's gradients of rank d's pieces of the bucket, +0.0 where a parameter has no gradient here).  The buffer is
        reused by the next call: move it on (or copy it) first."""
        if not self.shard_grads:
            raise RuntimeError("fused optimizer: pack_grad_bucket() belongs to shard_grads=True")
        gx = self._exchange()
        params = self._layout()[1]
        if not 0 <= k < gx["n"]:
            raise IndexError(f"fused optimizer: bucket {k} of {gx['n']}")
        if k == 0:  # once per micro-batch: the gradients that take part, checked
            present = [self._unfolded(p) for p in params]
            for p, here in zip(params, present):
                if here:
                    self._check_tensor(p, p.grad)
                    if p.grad.dtype != self._grad_dtype(p):
                        raise TypeError(f"fused optimizer: a gradient of dtype {p.grad.dtype} where {self._grad_dtype(p)} travels (set p.grad_dtype on every rank)")
            gx["present"] = present
        present, slot, send = gx["present"], gx["slot"], gx["send"]
        pieces = [(d, piece) for d, dest in enumerate(gx["grad"][k]) for piece in dest]
        live = [(d, piece) for d, piece in pieces if present[piece[0]]]
        if len(live) < len(pieces):
            send.zero_()  # what is absent here travels as +0.0
        table = (_lib.PrlSegment * max(len(live), 1))()
        for seg, (d, (i, b, e, at)) in zip(table, live):
            isz = gx["g_sizes"][i]
            seg.tensor, seg.bucket_offset, seg.nbytes = params[i].grad.data_ptr() + b * isz, d * slot + at, (e - b) * isz
        _lib.check(_lib.load().prl_bucket_gather(send.data_ptr(), send.numel(), table, len(live), _lib.current_stream_ptr(send.device)))
        return send

    @torch.no_grad()
    def fold_grad_bucket(self, k: int, received: torch.Tensor) -> None:
        """Second half: `received` is `world x slot` bytes, slot r = what rank r packed for THIS rank in bucket `k`; the `world` copies
        of every own piece are folded into its accumulator in rank order by one call (overwriting on the first micro-batch since the
        last step / `zero_grad()`)."""
        if not self.shard_grads:
            raise RuntimeError("fused optimizer: fold_grad_bucket() belongs to shard_grads=True")
        gx = self._exchange()
        (rank, world), slot = self._shard, gx["slot"]
        if not 0 <= k < gx["n"]:
            raise IndexError(f"fused optimizer: bucket {k} of {gx['n']}")
        if received.dtype != torch.uint8 or received.numel() != world * slot or not received.is_contiguous():
            raise ValueError(f"fused optimizer: fold_grad_bucket() takes {world} x {slot} contiguous bytes")
        _lib.require_device(received)
        self._ensure_accumulators()
        _, params, offsets, shard_len, _ = self._layout()
        mine = gx["grad"][k][rank]
        table = (_lib.PrlAccumRanksSegment * max(len(mine), 1))()
        base = self._acc_flat.data_ptr() - 4 * rank * shard_len
        for seg, (i, b, e, at) in zip(table, mine):
            seg.src, seg.acc, seg.numel = received.data_ptr() + at, base + 4 * (offsets[i] + b), e - b
            seg.src_dtype = _DTYPES[self._grad_dtype(params[i])]
        _lib.check(_lib.load().prl_optim_grad_accumulate_ranks(table, len(mine), world, slot, int(not self._folded), _lib.current_stream_ptr(received.device)))

    @torch.no_grad()
    def finish_grad_fold(self, set_to_none: bool = True) -> None:
        """Closes a micro-batch after its last bucket: clears `p.grad` (`set_to_none=False`: zeroed in place) and marks every own
        accumulator filled, so that the next micro-batch adds."""
        if not self.shard_grads:
            raise RuntimeError("fused optimizer: finish_grad_fold() belongs to shard_grads=True")
        self._ensure_accumulators()
        self._folded = True
        self._acc_filled.update(self._acc)
        for p in self._layout()[1]:
            if p.grad is None:
                continue
            if set_to_none:
                p.grad = None  # (freed in stream order: the gathers above have been enqueued)
                self._acc_zeroed.pop(p, None)
            elif self._unfolded(p):
                p.grad.zero_()
                self._acc_zeroed[p] = (p.grad, p.grad._version)

    def _accumulate_grads_sharded(self, set_to_none: bool) -> None:
        """`accumulate_grads()` with sharded gradients: a COLLECTIVE.  Every rank of the group calls it once per micro-batch, also a rank
        that has nothing to fold (its zeros are what the owners add) - the sentinel batches of the learner steps already make the
        ranks run equal numbers of forward / backward passes.  Per bucket: gather, `all_to_all_single` (slot d goes to rank d; RCCL
        and gloo alike), one fold of the `world` received copies.  Stream-ordered on the current stream and single-buffered: the next
        bucket's gather waits for this bucket's exchange (overlapping the two on a second buffer is a later step)."""
        import torch.distributed as dist

        if self._shard_group is None:
            raise RuntimeError("fused optimizer: shard= has no group to exchange the buckets over; move the data between pack_grad_bucket(k) and "
                               "fold_grad_bucket(k, received), then finish_grad_fold()")
        if dist.get_world_size(self._shard_group) != self._shard[1]:
            raise RuntimeError(f"fused optimizer: the state is sharded over {self._shard[1]} ranks, the group has {dist.get_world_size(self._shard_group)}")
        recv = self._exchange()["recv"]
        for k in range(self.n_grad_buckets()):
            send = self.pack_grad_bucket(k)
            dist.all_to_all_single(recv, send, group=self._shard_group)
            self.fold_grad_bucket(k, recv)
        self.finish_grad_fold(set_to_none)

    def _reduce_sharded_grads(self) -> None:
        """`reduce_accumulated()` with sharded gradients moves no data (the owners already hold the sums): the own range is divided by
        the world size and the step counts as reduced.  Nothing folded since the last step: the gradients are zero."""
        self._check_all_folded()
        self._ensure_accumulators()
        if self._acc_flat is None:
            return
        if not self._folded:
            self._acc_flat.zero_()
            self._acc_filled.update(self._acc)
        self._acc_flat.div_(self._shard[1])
        self._reduced = True

    @torch.no_grad()
    def pack_shard_bucket(self, k: int) -> torch.Tensor:
        """Sharded gradients, the weight exchange bucket by bucket: this rank's pieces of bucket `k` of the parameters, as they stand,
        packed into the first slot of the send buffer (uint8, `slot` bytes, the same size on every rank)."""
        if not self.shard_grads:
            raise RuntimeError("fused optimizer: pack_shard_bucket() belongs to shard_grads=True")
        gx = self._exchange()
        params, slot = self._layout()[1], gx["slot"]
        if not 0 <= k < gx["n"]:
            raise IndexError(f"fused optimizer: bucket {k} of {gx['n']}")
        mine = gx["weight"][k][self._shard[0]]
        table = (_lib.PrlSegment * max(len(mine), 1))()
        for seg, (i, b, e, at) in zip(table, mine):
            isz = params[i].element_size()
            seg.tensor, seg.bucket_offset, seg.nbytes = params[i].data_ptr() + b * isz, at, (e - b) * isz
        send = gx["send"][:slot]
        _lib.check(_lib.load().prl_bucket_gather(send.data_ptr(), slot, table, len(mine), _lib.current_stream_ptr(send.device)))
        return send

    @torch.no_grad()
    def unpack_shard_bucket(self, k: int, gathered: torch.Tensor) -> None:
        """`gathered`: every rank's `pack_shard_bucket(k)` in rank order (world x slot bytes); the other ranks' pieces are written into
        the parameters, the own ones are already there."""
        if not self.shard_grads:
            raise RuntimeError("fused optimizer: unpack_shard_bucket() belongs to shard_grads=True")
        gx = self._exchange()
        params, slot, (rank, world) = self._layout()[1], gx["slot"], self._shard
        if not 0 <= k < gx["n"]:
            raise IndexError(f"fused optimizer: bucket {k} of {gx['n']}")
        if gathered.dtype != torch.uint8 or gathered.numel() != world * slot or not gathered.is_contiguous():
            raise ValueError(f"fused optimizer: unpack_shard_bucket() takes {world} x {slot} contiguous bytes")
        _lib.require_device(gathered)
        others = [(r, piece) for r, pieces in enumerate(gx["weight"][k]) if r != rank for piece in pieces]
        table = (_lib.PrlSegment * max(len(others), 1))()
        for seg, (r, (i, b, e, at)) in zip(table, others):
            isz = params[i].element_size()
            seg.tensor, seg.bucket_offset, seg.nbytes = params[i].data_ptr() + b * isz, r * slot + at, (e - b) * isz
        _lib.check(_lib.load().prl_bucket_scatter(gathered.data_ptr(), gathered.numel(), table, len(others), _lib.current_stream_ptr(gathered.device)))

    # ---- segment table ----------------------------------------------------------------------------------------------------
    def _check_tensor(self, p: torch.Tensor, g: torch.Tensor | None) -> None:
        _lib.require_device(p, g)
        if p.dtype not in _DTYPES or (g is not None and g.dtype not in _DTYPES):
            raise TypeError(f"fused optimizer: parameters and gradients must be float32 or bfloat16 (got {p.dtype}, {None if g is None else g.dtype})")
        if not p.is_contiguous() or (g is not None and (g.is_sparse or not g.is_contiguous())):
            raise ValueError("fused optimizer: parameters and gradients must be dense and contiguous")

    def _build_table(self) -> None:
        """(Re)build the pointer table; called when a data_ptr or the presence of a gradient changed."""
        entries = [(p, group) for group in self.param_groups for p in group["params"]]
        devices = {p.device for p, _ in entries}
        for p, _ in entries:
            self._check_tensor(p, self._grad_of(p))
        if len(devices) > 1:
            raise ValueError(f"fused optimizer: all parameters must live on one device (got {sorted(map(str, devices))})")
        self._ensure_state()
        everything = entries
        ordinals = list(range(len(everything)))  # a parameter's index in param_groups order: what its random bits are keyed on
        if self._shard is not None:  # one segment per owned piece; `entries` = the parameters this rank owns a piece of
            mine = self._layout()[4]
            ranges = [mine[i] for i in range(len(everything)) if i in mine]
            entries = [e for i, e in enumerate(everything) if i in mine]
            ordinals = [i for i in ordinals if i in mine]
        else:
            ranges = [(0, p.numel()) for p, _ in entries]
        table = (_lib.PrlOptimSegment * max(len(entries), 1))()
        for seg, (p, _), (b, e) in zip(table, entries, ranges):
            g = self._grad_of(p)
            st = self.state[p] if g is not None else {}
            seg.param, seg.numel, seg.param_dtype = p.data_ptr() + b * p.element_size(), e - b, _DTYPES[p.dtype]
            at = 0 if self.shard_grads and p in self._acc_filled else b * g.element_size() if g is not None else 0  # a sharded accumulator IS the piece
            seg.grad = g.data_ptr() + at if g is not None and p.numel() else None
            seg.grad_dtype = _DTYPES[g.dtype] if g is not None else _DTYPES[p.dtype]
            if g is not None:
                self._fill_state(seg, st)
        if self._compact:  # the same entries with the rounding fields; step / lr / weight_decay are copied before every launch
            self._compact_table = (_lib.PrlOptimCompactSegment * max(len(entries), 1))()
            stochastic = self.param_rounding == "stochastic"
            for seg, c, (p, _), (b, _e), ordinal in zip(table, self._compact_table, entries, ranges, ordinals):
                for name, _t in _lib.PrlOptimSegment._fields_:
                    setattr(c, name, getattr(seg, name))
                c.state_dtype = _DTYPES[self.state_dtype]
                sr = stochastic and p.dtype == torch.bfloat16 and not self._wants_master(p)
                c.param_rounding = _lib.PRL_ROUND_STOCHASTIC if sr else _lib.PRL_ROUND_NEAREST
                c.elem_offset, c.ordinal = b, ordinal
        self._norm_table = None
        if self._shard is not None and self.grad_accum_dtype is None:  # complete gradients on every rank: the norm reads them whole
            self._norm_table = (_lib.PrlOptimSegment * max(len(everything), 1))()
            for seg, (p, _) in zip(self._norm_table, everything):
                g = p.grad
                seg.numel, seg.param_dtype = p.numel(), _DTYPES[p.dtype]
                seg.grad = g.data_ptr() if g is not None and p.numel() else None
                seg.grad_dtype = _DTYPES[g.dtype] if g is not None else _DTYPES[p.dtype]
        self._table, self._table_params = table, entries
        owned = {id(p) for p, _ in entries}
        self._table_group_sizes = [sum(id(p) in owned for p in group["params"]) for group in self.param_groups]
        self._table_key, self._table_n_all = self._key(everything), len(everything)
        entries = everything
        if entries:
            device = self._device = entries[0][0].device
            if self._record is None:
                self._record = torch.zeros(2, dtype=torch.float32, device=device)
            need = ctypes.c_size_t(0)  # re-queried on every rebuild: add_param_group may have added elements
            _lib.check(_lib.load().prl_optim_workspace_bytes(len(entries), sum(p.numel() for p, _ in entries), ctypes.byref(need)))
            if self._workspace is None or self._workspace.numel() < need.value:
                self._workspace = torch.empty(max(need.value, 8), dtype=torch.uint8, device=device)

    def _fill_state(self, seg, st: dict) -> None:
        seg.exp_avg = st["exp_avg"].data_ptr()
        seg.exp_avg_sq = st["exp_avg_sq"].data_ptr() if "exp_avg_sq" in st else None
        seg.master = st["master"].data_ptr() if "master" in st else None

    def _key(self, entries) -> list[tuple]:
        grads = [self._grad_of(p) for p, _ in entries]  # an accumulator where one is filled: another address AND another dtype
        return [(p.data_ptr(), 0 if g is None else g.data_ptr(), None if g is None else g.dtype) for (p, _), g in zip(entries, grads)]

    def _current_table(self):
        entries = [(p, group) for group in self.param_groups for p in group["params"]]
        if self._table is None or len(entries) != self._table_n_all or self._key(entries) != self._table_key:
            self._build_table()
        return self._table, self._table_params

    def _stream(self) -> int:
        return _lib.current_stream_ptr(self._device)

    # ---- the public steps ---------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def compute_grad_norm(self, max_norm: float | None) -> torch.Tensor:
        """One pass over every gradient: the L2 norm and `min(1, max_norm / (norm + 1e-6))` into the device record the next
        `step(clipped=True)` reads.  Returns a 0-dim DEVICE tensor with the norm (a copy of the record's entry, so it keeps this
        step's value after the next norm pass; the caller decides when to `float()` it).
        `max_norm` None or <= 0 reports the norm and clips nothing."""
        lib = _lib.load()
        self._check_all_folded()
        if self._shard is not None and self.grad_accum_dtype is not None:
            # no rank holds every reduced gradient: shard partials, one fp64 all_reduce, the record from the total - stream-ordered
            if self._shard_group is None:
                raise RuntimeError("fused optimizer: shard= has no group to add the partial sums over; use local_grad_sumsq() and norm_from_sumsq()")
            import torch.distributed as dist

            sumsq = self.local_grad_sumsq()
            dist.all_reduce(sumsq, op=dist.ReduceOp.SUM, group=self._shard_group)
            return self.norm_from_sumsq(sumsq, max_norm)
        table, entries = self._current_table()
        if not self._table_n_all:
            raise ValueError("fused optimizer: no parameters")
        if self._norm_table is not None:
            table, entries = self._norm_table, range(self._table_n_all)
        _lib.check(lib.prl_optim_grad_norm(table, len(entries), 0.0 if max_norm is None else float(max_norm), self._workspace.data_ptr(),
                                           self._workspace.numel(), self._record.data_ptr(), self._stream()))
        return self._record[0].clone()

    def _check_reduced(self) -> None:
        if self._shard is not None and self.grad_accum_dtype is not None and not self._reduced:
            raise RuntimeError("fused optimizer: the sharded accumulators were not reduced since the last step; call reduce_accumulated() first")

    @torch.no_grad()
    def local_grad_sumsq(self) -> torch.Tensor:
        """Sharded fp32 accumulation: the fp64 sum of squares of the reduced gradients of this rank's pieces, on the device
        (a 1-element tensor that the next call overwrites).  The ranks' values are added, then `norm_from_sumsq`."""
        if self._shard is None or self.grad_accum_dtype is None:
            raise RuntimeError("fused optimizer: local_grad_sumsq() belongs to sharded state with grad_accum_dtype=torch.float32")
        self._check_all_folded()
        self._check_reduced()
        table, entries = self._current_table()
        if not self._table_n_all:
            raise ValueError("fused optimizer: no parameters")
        if self._sumsq is None:
            self._sumsq = torch.zeros(1, dtype=torch.float64, device=self._device)
        _lib.check(_lib.load().prl_optim_grad_sumsq(table, len(entries), self._workspace.data_ptr(), self._workspace.numel(), self._sumsq.data_ptr(),
                                                    self._stream()))
        return self._sumsq

    @torch.no_grad()
    def norm_from_sumsq(self, sumsq: torch.Tensor, max_norm: float | None) -> torch.Tensor:
        """Norm and clip coefficient from the sum of squares over ALL ranks (device, fp64) into the record `step(clipped=True)` reads."""
        if sumsq.dtype != torch.float64 or not sumsq.is_cuda or sumsq.numel() != 1:
            raise ValueError("fused optimizer: norm_from_sumsq() takes one float64 value on the device")
        self._current_table()
        _lib.check(_lib.load().prl_optim_clip_from_sumsq(sumsq.data_ptr(), 0.0 if max_norm is None else float(max_norm), self._record.data_ptr(),
                                                         self._stream()))
        return self._record[0].clone()

    def clip_and_step(self, max_norm: float | None) -> torch.Tensor:
        """`clip_grad_norm_(parameters, max_norm)` + `step()` with the coefficient consumed on the device; step hooks fire.
        Returns the total norm as a 0-dim device tensor.  The gradients keep their unclipped values."""
        norm = self.compute_grad_norm(max_norm)
        self.step(clipped=True)
        return norm

    @torch.no_grad()
    def step(self, closure=None, *, clipped: bool = False):
        """Plain step; `clipped=True` scales every gradient by the coefficient of the last `compute_grad_norm`."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = _lib.load()
        self._check_all_folded()
        self._check_reduced()
        table, entries = self._current_table()
        if not self._table_n_all:
            return loss
        for seg, (p, group) in zip(table, entries):
            if self._grad_of(p) is None:
                continue
            st = self.state[p]
            st["step"] += 1
            seg.step = int(st["step"])
            seg.lr, seg.weight_decay = float(group["lr"]), float(group["weight_decay"])
        self._launch(lib, table, len(entries), self._record.data_ptr() if clipped else None)
        self._acc_filled.clear()  # the next fold of every accumulator overwrites
        self._reduced = False
        self._folded = False
        if self._shard_group is not None:
            self._exchange_weights()
        return loss

    # ---- sharded: publishing the updated pieces ---------------------------------------------------------------------------
    def _publish_buffers(self):
        """Byte layout of every rank's send buffer (the same on every rank): its pieces in plan order, each at a 16-byte aligned
        offset, the buffer padded to the largest rank's size.  Allocated once."""
        if self._pub is None:
            numels, params, _, _, _ = self._layout()
            per_rank, size = [], 0
            for pieces in plan_shards(numels, self._shard[1]):
                off, segs = 0, []
                for i, b, e in pieces:
                    isz = params[i].element_size()
                    segs.append((i, b * isz, (e - b) * isz, off))
                    off += -(-(e - b) * isz // 16) * 16
                per_rank.append(segs)
                size = max(size, off)
            size = max(size, 16)
            device = params[0].device
            self._pub = (per_rank, size, torch.zeros(size, dtype=torch.uint8, device=device), torch.zeros(self._shard[1] * size, dtype=torch.uint8, device=device))
        return self._pub

    def _publish_tables(self):
        """`prl_segment` tables of the exchange: own pieces -> send buffer, the other ranks' pieces <- receive buffer; rebuilt when a
        parameter moved."""
        per_rank, size, _, _ = self._publish_buffers()
        params = self._layout()[1]
        key = [p.data_ptr() for p in params]
        if self._pub_tables is None or self._pub_tables[0] != key:
            rank = self._shard[0]
            out = (_lib.PrlSegment * max(len(per_rank[rank]), 1))()
            for seg, (i, at, nbytes, off) in zip(out, per_rank[rank]):
                seg.tensor, seg.bucket_offset, seg.nbytes = params[i].data_ptr() + at, off, nbytes
            others = [(r, piece) for r, pieces in enumerate(per_rank) if r != rank for piece in pieces]
            inn = (_lib.PrlSegment * max(len(others), 1))()
            for seg, (r, (i, at, nbytes, off)) in zip(inn, others):
                seg.tensor, seg.bucket_offset, seg.nbytes = params[i].data_ptr() + at, r * size + off, nbytes
            self._pub_tables = (key, out, len(per_rank[rank]), inn, len(others))
        return self._pub_tables

    @torch.no_grad()
    def pack_shard(self) -> torch.Tensor:
        """This rank's pieces of the parameters, as they stand, packed into its send buffer (uint8, the same size on every rank)."""
        self._no_whole_buffer("pack_shard() / unpack_shards()", "pack_shard_bucket(k) / unpack_shard_bucket(k, gathered) for k in range(n_grad_buckets())")
        _, size, send, _ = self._publish_buffers()
        _, out, n_out, _, _ = self._publish_tables()
        _lib.check(_lib.load().prl_bucket_gather(send.data_ptr(), size, out, n_out, _lib.current_stream_ptr(send.device)))
        return send

    @torch.no_grad()
    def unpack_shards(self, gathered: torch.Tensor) -> None:
        """`gathered`: every rank's send buffer in rank order (world x size bytes); the other ranks' pieces are written into the
        parameters, the own ones are already there."""
        self._no_whole_buffer("pack_shard() / unpack_shards()", "pack_shard_bucket(k) / unpack_shard_bucket(k, gathered) for k in range(n_grad_buckets())")
        _, size, _, _ = self._publish_buffers()
        _, _, _, inn, n_in = self._publish_tables()
        if gathered.dtype != torch.uint8 or gathered.numel() != self._shard[1] * size or not gathered.is_contiguous():
            raise ValueError(f"fused optimizer: unpack_shards() takes {self._shard[1]} x {size} contiguous bytes")
        _lib.require_device(gathered)
        _lib.check(_lib.load().prl_bucket_scatter(gathered.data_ptr(), gathered.numel(), inn, n_in, _lib.current_stream_ptr(gathered.device)))

    def _exchange_weights(self) -> None:
        import torch.distributed as dist

        if self.shard_grads:  # bucket by bucket through the exchange buffers: no whole-model receive buffer
            gx = self._exchange()
            nccl = dist.get_backend(self._shard_group) == "nccl"
            for k in range(gx["n"]):
                send = self.pack_shard_bucket(k)
                if nccl:
                    dist.all_gather_into_tensor(gx["recv"], send, group=self._shard_group)
                else:
                    dist.all_gather(list(gx["recv"].view(self._shard[1], -1).unbind(0)), send, group=self._shard_group)
                self.unpack_shard_bucket(k, gx["recv"])
            return
        _, _, _, recv = self._publish_buffers()
        send = self.pack_shard()
        if dist.get_backend(self._shard_group) == "nccl":
            dist.all_gather_into_tensor(recv, send, group=self._shard_group)
        else:
            dist.all_gather(list(recv.view(self._shard[1], -1).unbind(0)), send, group=self._shard_group)
        self.unpack_shards(recv)

    def _launch(self, lib, table, n: int, record: int | None) -> None:
        """One call per run of consecutive groups that agree on the launch-level constants (betas, eps): normally one."""
        if self._compact:
            for seg, c in zip(table, self._compact_table):
                c.step, c.lr, c.weight_decay = seg.step, seg.lr, seg.weight_decay
            table = self._compact_table
        sizes = self._table_group_sizes  # the table's entries per group (sharded: the parameters this rank owns a piece of)
        keys = [self._launch_key(g) for g in self.param_groups]
        first, off = 0, 0
        for i in range(len(sizes)):
            if i + 1 < len(sizes) and keys[i + 1] == keys[first]:
                continue
            k = sum(sizes[first:i + 1])
            if k:
                sub = ctypes.byref(table, off * ctypes.sizeof(self._segment_type))
                self._call(lib, sub, k, keys[first], record)
            off += k
            first = i + 1

    def _launch_key(self, group: dict) -> tuple:
        raise NotImplementedError

    def _call(self, lib, table, n: int, key: tuple, record: int | None) -> None:
        raise NotImplementedError


class FusedAdamW(_FusedOptimizer):
    """`torch.optim.AdamW` (amsgrad off) as one fused launch per 32 parameters; fp32 state, optional fp32 master weights.
    `state_dtype=torch.bfloat16`: bf16 moments stored with stochastic rounding; `param_rounding="stochastic"`: a bf16 parameter
    without a master copy is written with stochastic rounding; `seed` keys the random bits (module docstring)."""

    _state_keys = ("exp_avg", "exp_avg_sq")

    def __init__(self, params, lr: float = 1e-3, betas: tuple[float, float] = (0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2,
                 master_weights: bool = True, grad_accum_dtype: torch.dtype | None = None, shard_group=None, shard: tuple[int, int] | None = None,
                 state_dtype: torch.dtype | None = None, param_rounding: str = "nearest", seed: int = 0, shard_grads: bool = False,
                 exchange_bucket_bytes: int = 64 << 20):
        _check_hyper(lr, betas, weight_decay, eps)
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, seed=seed), master_weights, grad_accum_dtype, shard_group,
                         shard, state_dtype, param_rounding, shard_grads, exchange_bucket_bytes)

    def _launch_key(self, group):
        return (float(group["betas"][0]), float(group["betas"][1]), float(group["eps"]), int(group.get("seed", 0)))

    def _call(self, lib, table, n, key, record):
        if self._compact:
            _lib.check(lib.prl_optim_adamw_step_compact(table, n, key[0], key[1], key[2], key[3], record, self._stream()))
        else:
            _lib.check(lib.prl_optim_adamw_step(table, n, key[0], key[1], key[2], record, self._stream()))


class FusedLion(_FusedOptimizer):
    """The reference's `Lion` (pipelinerl/finetune/optim.py:48-112) as one fused launch per 32 parameters.  `state_dtype`,
    `param_rounding`, `seed`: compact state as in `FusedAdamW`."""

    _state_keys = ("exp_avg",)

    def __init__(self, params, lr: float = 1e-4, betas: tuple[float, float] = (0.9, 0.99), weight_decay: float = 0.0, master_weights: bool = True,
                 grad_accum_dtype: torch.dtype | None = None, shard_group=None, shard: tuple[int, int] | None = None,
                 state_dtype: torch.dtype | None = None, param_rounding: str = "nearest", seed: int = 0, shard_grads: bool = False,
                 exchange_bucket_bytes: int = 64 << 20):
        _check_hyper(lr, betas, weight_decay)
        super().__init__(params, dict(lr=lr, betas=betas, weight_decay=weight_decay, seed=seed), master_weights, grad_accum_dtype, shard_group, shard,
                         state_dtype, param_rounding, shard_grads, exchange_bucket_bytes)

    def _launch_key(self, group):
        return (float(group["betas"][0]), float(group["betas"][1]), int(group.get("seed", 0)))

    def _call(self, lib, table, n, key, record):
        if self._compact:
            _lib.check(lib.prl_optim_lion_step_compact(table, n, key[0], key[1], key[2], record, self._stream()))
        else:
            _lib.check(lib.prl_optim_lion_step(table, n, key[0], key[1], record, self._stream()))


class FusedAdafactor(_FusedOptimizer):
    """transformers' `Adafactor(relative_step=False, scale_parameter=False)` - what the reference builds for "adafactor" - as six
    fused launches per 32 parameters (csrc/prl_adafactor.hip): factored second moments for every parameter with two or more
    dimensions (the leading ones are a batch of matrices), the update clipped by its own rms over the whole parameter.  fp32
    state under transformers' keys (`step`, `exp_avg_sq_row`, `exp_avg_sq_col` or `exp_avg_sq`; `RMS`, which the rule never reads,
    is not kept) plus `master` for bf16 parameters; a `transformers.Adafactor` `state_dict()` over the same parameters loads (the
    master copy is then seeded from the parameter), and this class's state without `master` loads into `transformers.Adafactor`.
    The boundary protocol is the fused optimizers': `accumulate_grads`, `reduce_accumulated`, `compute_grad_norm`, `clip_and_step`.
    `beta1`, `relative_step` and `scale_parameter` are not built, and neither is sharded state: row and column averages do not cut
    into element ranges."""

    _state_keys = ("exp_avg_sq_row", "exp_avg_sq_col", "exp_avg_sq")  # every key a parameter can have: `_keys_of` picks

    def __init__(self, params, lr: float = 1e-3, eps1: float = 1e-30, clip_threshold: float = 1.0, decay_rate: float = -0.8, weight_decay: float = 0.0,
                 master_weights: bool = True, grad_accum_dtype: torch.dtype | None = None, beta1=None, relative_step: bool = False,
                 scale_parameter: bool = False, shard_group=None, shard: tuple[int, int] | None = None, state_dtype: torch.dtype | None = None,
                 param_rounding: str = "nearest", seed: int = 0, shard_grads: bool = False):
        if shard_grads:
            raise ValueError("FusedAdafactor: sharded gradients (shard_grads) are not built for Adafactor (it has no sharded state to go with them)")
        if state_dtype not in (None, torch.float32) or param_rounding != "nearest" or seed != 0:
            raise ValueError("FusedAdafactor: compact state (state_dtype, param_rounding, seed) is not built for Adafactor (its factored averages are tiny)")
        unsupported = [n for n, on in (("beta1", beta1 is not None), ("relative_step", relative_step), ("scale_parameter", scale_parameter)) if on]
        if unsupported:
            raise ValueError(f"FusedAdafactor: {', '.join(unsupported)} not supported (the fused step is the reference's rule: beta1=None, "
                             "relative_step=False, scale_parameter=False)")
        if shard_group is not None or shard is not None:
            raise ValueError("FusedAdafactor: sharded optimizer state is not built for Adafactor (row and column averages do not cut into element ranges)")
        if lr is None or not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps1:
            raise ValueError(f"Invalid epsilon value: {eps1}")
        if not 0.0 < clip_threshold:
            raise ValueError(f"Invalid clip_threshold value: {clip_threshold}")
        if not decay_rate <= 0.0:
            raise ValueError(f"Invalid decay_rate value: {decay_rate}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        # transformers' group keys, so that a state dictionary travels both ways (eps[1] belongs to scale_parameter and is never read)
        defaults = dict(lr=lr, eps=(eps1, 1e-3), clip_threshold=clip_threshold, decay_rate=decay_rate, beta1=None, weight_decay=weight_decay,
                        scale_parameter=False, relative_step=False, warmup_init=False)
        super().__init__(params, defaults, master_weights, grad_accum_dtype)
        self._ada_table = None
        self._ada_workspace: torch.Tensor | None = None

    @staticmethod
    def _factored(p: torch.Tensor) -> bool:
        return p.dim() >= 2

    def _keys_of(self, p):
        keys = ("exp_avg_sq_row", "exp_avg_sq_col") if self._factored(p) else ("exp_avg_sq",)
        return keys + (("master",) if self._wants_master(p) else ())

    def _state_shape(self, p, key):
        if key == "exp_avg_sq_row":
            return p.shape[:-1]
        if key == "exp_avg_sq_col":
            return p.shape[:-2] + p.shape[-1:]
        return p.shape

    def _fill_state(self, seg, st):
        pass  # the norm pass reads gradients only; the step has its own table

    def load_state_dict(self, state_dict: dict) -> None:
        super().load_state_dict(state_dict)
        for group in self.param_groups:
            if group.get("beta1") is not None or group.get("relative_step") or group.get("scale_parameter"):
                raise ValueError("FusedAdafactor: the loaded param_groups use beta1, relative_step or scale_parameter, which are not supported")
        for st in self.state.values():
            st.pop("RMS", None)
        self._ada_table = None

    def _build_table(self) -> None:
        super()._build_table()
        entries = self._table_params
        table = (_lib.PrlAdafactorSegment * max(len(entries), 1))()
        for seg, (p, _) in zip(table, entries):
            g = self._grad_of(p)
            seg.param, seg.param_dtype = p.data_ptr(), _DTYPES[p.dtype]
            seg.grad = g.data_ptr() if g is not None and p.numel() else None
            seg.grad_dtype = _DTYPES[g.dtype] if g is not None else _DTYPES[p.dtype]
            if self._factored(p):
                seg.rows, seg.cols = p.shape[-2], p.shape[-1]
                seg.batch = p.numel() // (seg.rows * seg.cols) if seg.rows * seg.cols else 0
            else:
                seg.batch, seg.rows, seg.cols = 1, 1, p.numel()
            if g is not None:
                st = self.state[p]
                seg.row = st["exp_avg_sq_row"].data_ptr() if "exp_avg_sq_row" in st else None
                seg.col = st["exp_avg_sq_col"].data_ptr() if "exp_avg_sq_col" in st else None
                seg.v = st["exp_avg_sq"].data_ptr() if "exp_avg_sq" in st else None
                seg.master = st["master"].data_ptr() if "master" in st else None
                seg.step = 1  # (the table is sized with a valid step; the real one is written before every launch)
        self._ada_table = table
        if entries:
            need = ctypes.c_size_t(0)
            _lib.check(_lib.load().prl_adafactor_workspace_bytes(table, len(entries), ctypes.byref(need)))
            if self._ada_workspace is None or self._ada_workspace.numel() < need.value:
                self._ada_workspace = torch.empty(max(need.value, 16), dtype=torch.uint8, device=self._device)

    def _launch(self, lib, table, n: int, record: int | None) -> None:
        """One call per run of consecutive groups that agree on the launch-level constants (eps1, clip_threshold, decay_rate)."""
        for seg, ada in zip(table, self._ada_table):
            ada.step, ada.lr, ada.weight_decay = seg.step, seg.lr, seg.weight_decay
        super()._launch(lib, self._ada_table, n, record)

    _segment_type = _lib.PrlAdafactorSegment

    def _launch_key(self, group):
        return (float(group["eps"][0]), float(group["clip_threshold"]), float(group["decay_rate"]))

    def _call(self, lib, table, n, key, record):
        _lib.check(lib.prl_adafactor_step(table, n, key[0], key[1], key[2], record, self._ada_workspace.data_ptr(), self._ada_workspace.numel(), self._stream()))


def get_optimizer(name: str, model: torch.nn.Module, learning_rate: float, weight_decay: float, grad_accum_dtype: torch.dtype | None = None,
                  shard_group=None, shard: tuple[int, int] | None = None, state_dtype: torch.dtype | None = None, param_rounding: str = "nearest",
                  seed: int = 0, shard_grads: bool = False, exchange_bucket_bytes: int = 64 << 20):
    """The reference's dispatch (:25-45) with its names; "adamw_torch" and "lion" are the fused HIP steps, "adafactor_hip" is the
    fused HIP form of "adafactor" (which stays transformers' class).
    `grad_accum_dtype=torch.float32`: fp32 gradient accumulation (the fused steps only); `shard_group` / `shard`: state sharded over
    the learner ranks ("adamw_torch" and "lion" only); `state_dtype` / `param_rounding` / `seed`: compact state with stochastic rounding
    ("adamw_torch" and "lion" only); `shard_grads` / `exchange_bucket_bytes`: the fp32 accumulators sharded like the state, gradients and
    weights exchanged in buckets ("adamw_torch" and "lion" only)."""
    grouped_params = get_grouped_params(model, weight_decay)
    compact = dict(state_dtype=state_dtype, param_rounding=param_rounding, seed=seed, shard_grads=shard_grads, exchange_bucket_bytes=exchange_bucket_bytes)
    if (shard_grads or exchange_bucket_bytes != 64 << 20) and name not in ("adamw_torch", "lion"):
        raise ValueError(f'sharded gradients (shard_grads, exchange_bucket_bytes) need "adamw_torch" or "lion", not "{name}"')
    if (state_dtype not in (None, torch.float32) or param_rounding != "nearest" or seed != 0) and name not in ("adamw_torch", "lion"):
        raise ValueError(f'compact optimizer state (state_dtype, param_rounding, seed) needs "adamw_torch" or "lion", not "{name}"')
    if name == "adafactor_hip":
        return FusedAdafactor(grouped_params, lr=learning_rate, grad_accum_dtype=grad_accum_dtype, shard_group=shard_group, shard=shard)
    if grad_accum_dtype is not None and name not in ("adamw_torch", "lion"):
        raise ValueError(f'grad_accum_dtype needs a fused optimizer ("adamw_torch" or "lion"), not "{name}"')
    if (shard_group is not None or shard is not None) and name not in ("adamw_torch", "lion"):
        raise ValueError(f'sharded optimizer state needs a fused optimizer ("adamw_torch" or "lion"), not "{name}"')
    if name == "adamw_torch":
        return FusedAdamW(grouped_params, lr=learning_rate, grad_accum_dtype=grad_accum_dtype, shard_group=shard_group, shard=shard, **compact)
    if name == "adafactor":
        from transformers import Adafactor

        return Adafactor(grouped_params, lr=learning_rate, relative_step=False, scale_parameter=False)
    if name == "cpuadam":
        try:
            import deepspeed.ops.adam
        except ImportError as e:
            raise ImportError(f'optimizer "cpuadam" needs the deepspeed package: {e}') from e
        return deepspeed.ops.adam.DeepSpeedCPUAdam(grouped_params, lr=learning_rate)
    if name == "lion":
        return FusedLion(grouped_params, lr=learning_rate, grad_accum_dtype=grad_accum_dtype, shard_group=shard_group, shard=shard, **compact)
    raise ValueError(f"Unknown optimizer: {name}")
