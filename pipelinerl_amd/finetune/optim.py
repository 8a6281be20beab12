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
the norm computed here is complete on every rank.  ZeRO / FSDP sharded norms are out of scope.

Gradient accumulation (`grad_accum_dtype=torch.float32`): autograd sums the micro-batch gradients into `p.grad` in the
parameter's dtype, and a bf16 running sum drops every term below half an ulp of it - after 256 equal terms all of the next one.
The reference accumulates in fp32 (FSDP `param_dtype / reduce_dtype: fp32`, DeepSpeed's fp32 gradient partitions).  With the
option, `accumulate_grads()` after every `backward()` folds each bf16 `p.grad` into an fp32 accumulator (one IEEE add per
element and micro-batch, `prl_optim_grad_accumulate`) and clears `p.grad`; norm and step read the accumulators;
`reduce_accumulated(group)` averages them over the data-parallel ranks in fp32 (run every pass under `no_sync()`: DDP would
reduce the last micro-batch's `p.grad` only).  fp32 gradients (the fp32 `lm_head`, which the fused head already accumulates
into in fp32) are used as they are.  The accumulators are views of one flat buffer, transient (not in `state_dict()`), and
cost 4 bytes per bf16 element: 28 GB on the Qwen2.5-7B list.

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


class _FusedOptimizer(torch.optim.Optimizer):
    """Shared host side of the fused steps: lazily allocated flat fp32 state, the segment table, the norm record."""

    _state_keys: tuple[str, ...] = ("exp_avg",)

    def __init__(self, params: Iterable, defaults: dict[str, Any], master_weights: bool, grad_accum_dtype: torch.dtype | None = None):
        if grad_accum_dtype not in (None, torch.float32):
            raise ValueError(f"fused optimizer: grad_accum_dtype must be None or torch.float32 (got {grad_accum_dtype})")
        super().__init__(params, defaults)
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

    def _is_flat_view(self, t: torch.Tensor) -> bool:
        return any(t.untyped_storage().data_ptr() == f.untyped_storage().data_ptr() for f in self._flat)

    def _ensure_state(self) -> None:
        """State of every parameter that has a gradient and none yet (or a loaded one that is not in a flat buffer)."""
        for group in self.param_groups:
            todo = []
            for p in group["params"]:
                if self._grad_of(p) is None:
                    continue
                st = self.state[p]
                keys = self._keys_of(p)
                if all(k in st and st[k].dtype == torch.float32 and st[k].device == p.device and self._is_flat_view(st[k]) for k in keys) and "step" in st:
                    continue
                todo.append(p)
            if not todo:
                continue
            device = todo[0].device
            for key in self._state_keys + ("master",):
                owners = [p for p in todo if key in self._keys_of(p)]
                if not owners:
                    continue
                slots = [(-(-p.numel() // _SLOT)) * _SLOT for p in owners]
                flat = torch.zeros(sum(slots), dtype=torch.float32, device=device)
                self._flat.append(flat)
                off = 0
                for p, slot in zip(owners, slots):
                    view = flat[off:off + p.numel()].view(p.shape)
                    off += slot
                    st = self.state[p]
                    if key in st:  # loaded from a checkpoint: keep its values
                        view.copy_(st[key].to(device=device, dtype=torch.float32).reshape(p.shape))
                    elif key == "master":
                        view.copy_(p.detach())
                    st[key] = view
            for p in todo:
                self.state[p].setdefault("step", torch.tensor(0.0, dtype=torch.float32))
        self._flat = [f for f in self._flat if any(self._owns(f, st) for st in self.state.values())]

    @staticmethod
    def _owns(flat: torch.Tensor, st: dict) -> bool:
        ptr = flat.untyped_storage().data_ptr()
        return any(isinstance(v, torch.Tensor) and v.numel() and v.untyped_storage().data_ptr() == ptr for v in st.values())

    def load_state_dict(self, state_dict: dict) -> None:
        """torch casts loaded state to the parameter's dtype; the state here is fp32 whatever the parameter is, so the saved
        tensors are taken as they are (a torch.optim.AdamW checkpoint of fp32 parameters loads: same keys)."""
        super().load_state_dict(state_dict)
        saved_ids = [i for g in state_dict["param_groups"] for i in g["params"]]
        ours = [p for g in self.param_groups for p in g["params"]]
        for pid, p in zip(saved_ids, ours):
            src = state_dict["state"].get(pid)
            if src is None:
                continue
            for k in self._state_keys + ("master",):
                if k in src:
                    self.state[p][k] = src[k].detach().to(device=p.device, dtype=torch.float32).clone()
            if "step" in src:
                self.state[p]["step"] = torch.as_tensor(src["step"], dtype=torch.float32).detach().cpu().clone()
        self._flat, self._table, self._table_key = [], None, []

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

    def _unfolded(self, p: torch.Tensor) -> bool:
        g = p.grad
        if g is None or g.dtype == torch.float32:
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

    @torch.no_grad()
    def accumulate_grads(self, set_to_none: bool = True) -> None:
        """Call after every micro-batch's `backward()`: folds each present non-fp32 `p.grad` into its fp32 accumulator
        (`acc = g.float()` on a parameter's first fold since the last step / `zero_grad()`, `acc += g.float()` afterwards, one fp32
        add per element) and sets `p.grad = None`, so that the next backward moves its gradient in instead of adding to a stale one
        (`set_to_none=False`: zeroed in place).  fp32 gradients are left alone: they already accumulate in fp32."""
        if self.grad_accum_dtype is None:
            raise RuntimeError("fused optimizer: accumulate_grads() needs grad_accum_dtype=torch.float32")
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

    def zero_grad(self, set_to_none: bool = True) -> None:
        """Clears `p.grad` as torch does and marks every accumulator empty (no memset: the next fold overwrites)."""
        super().zero_grad(set_to_none=set_to_none)
        self._acc_filled.clear()
        self._acc_zeroed.clear()

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
        table = (_lib.PrlOptimSegment * max(len(entries), 1))()
        for seg, (p, _) in zip(table, entries):
            g = self._grad_of(p)
            st = self.state[p] if g is not None else {}
            seg.param, seg.numel, seg.param_dtype = p.data_ptr(), p.numel(), _DTYPES[p.dtype]
            seg.grad = g.data_ptr() if g is not None and p.numel() else None
            seg.grad_dtype = _DTYPES[g.dtype] if g is not None else _DTYPES[p.dtype]
            if g is not None:
                seg.exp_avg = st["exp_avg"].data_ptr()
                seg.exp_avg_sq = st["exp_avg_sq"].data_ptr() if "exp_avg_sq" in st else None
                seg.master = st["master"].data_ptr() if "master" in st else None
        self._table, self._table_params = table, entries
        self._table_key = self._key(entries)
        if entries:
            device = entries[0][0].device
            if self._record is None:
                self._record = torch.zeros(2, dtype=torch.float32, device=device)
            need = ctypes.c_size_t(0)  # re-queried on every rebuild: add_param_group may have added elements
            _lib.check(_lib.load().prl_optim_workspace_bytes(len(entries), sum(p.numel() for p, _ in entries), ctypes.byref(need)))
            if self._workspace is None or self._workspace.numel() < need.value:
                self._workspace = torch.empty(max(need.value, 8), dtype=torch.uint8, device=device)

    def _key(self, entries) -> list[tuple]:
        grads = [self._grad_of(p) for p, _ in entries]  # an accumulator where one is filled: another address AND another dtype
        return [(p.data_ptr(), 0 if g is None else g.data_ptr(), None if g is None else g.dtype) for (p, _), g in zip(entries, grads)]

    def _current_table(self):
        entries = [(p, group) for group in self.param_groups for p in group["params"]]
        if self._table is None or len(entries) != len(self._table_params) or self._key(entries) != self._table_key:
            self._build_table()
        return self._table, self._table_params

    def _stream(self) -> int:
        return _lib.current_stream_ptr(self._table_params[0][0].device)

    # ---- the public steps ---------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def compute_grad_norm(self, max_norm: float | None) -> torch.Tensor:
        """One pass over every gradient: the L2 norm and `min(1, max_norm / (norm + 1e-6))` into the device record the next
        `step(clipped=True)` reads.  Returns a 0-dim DEVICE tensor with the norm (a copy of the record's entry, so it keeps this
        step's value after the next norm pass; the caller decides when to `float()` it).
        `max_norm` None or <= 0 reports the norm and clips nothing."""
        lib = _lib.load()
        self._check_all_folded()
        table, entries = self._current_table()
        if not entries:
            raise ValueError("fused optimizer: no parameters")
        _lib.check(lib.prl_optim_grad_norm(table, len(entries), 0.0 if max_norm is None else float(max_norm), self._workspace.data_ptr(),
                                           self._workspace.numel(), self._record.data_ptr(), self._stream()))
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
        table, entries = self._current_table()
        if not entries:
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
        return loss

    def _launch(self, lib, table, n: int, record: int | None) -> None:
        """One call per run of consecutive groups that agree on the launch-level constants (betas, eps): normally one."""
        sizes = [len(g["params"]) for g in self.param_groups]
        keys = [self._launch_key(g) for g in self.param_groups]
        first, off = 0, 0
        for i in range(len(sizes)):
            if i + 1 < len(sizes) and keys[i + 1] == keys[first]:
                continue
            k = sum(sizes[first:i + 1])
            if k:
                sub = ctypes.byref(table, off * ctypes.sizeof(_lib.PrlOptimSegment))
                self._call(lib, sub, k, keys[first], record)
            off += k
            first = i + 1

    def _launch_key(self, group: dict) -> tuple:
        raise NotImplementedError

    def _call(self, lib, table, n: int, key: tuple, record: int | None) -> None:
        raise NotImplementedError


class FusedAdamW(_FusedOptimizer):
    """`torch.optim.AdamW` (amsgrad off) as one fused launch per 32 parameters; fp32 state, optional fp32 master weights."""

    _state_keys = ("exp_avg", "exp_avg_sq")

    def __init__(self, params, lr: float = 1e-3, betas: tuple[float, float] = (0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2,
                 master_weights: bool = True, grad_accum_dtype: torch.dtype | None = None):
        _check_hyper(lr, betas, weight_decay, eps)
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay), master_weights, grad_accum_dtype)

    def _launch_key(self, group):
        return (float(group["betas"][0]), float(group["betas"][1]), float(group["eps"]))

    def _call(self, lib, table, n, key, record):
        _lib.check(lib.prl_optim_adamw_step(table, n, key[0], key[1], key[2], record, self._stream()))


class FusedLion(_FusedOptimizer):
    """The reference's `Lion` (pipelinerl/finetune/optim.py:48-112) as one fused launch per 32 parameters."""

    _state_keys = ("exp_avg",)

    def __init__(self, params, lr: float = 1e-4, betas: tuple[float, float] = (0.9, 0.99), weight_decay: float = 0.0, master_weights: bool = True,
                 grad_accum_dtype: torch.dtype | None = None):
        _check_hyper(lr, betas, weight_decay)
        super().__init__(params, dict(lr=lr, betas=betas, weight_decay=weight_decay), master_weights, grad_accum_dtype)

    def _launch_key(self, group):
        return (float(group["betas"][0]), float(group["betas"][1]))

    def _call(self, lib, table, n, key, record):
        _lib.check(lib.prl_optim_lion_step(table, n, key[0], key[1], record, self._stream()))


def get_optimizer(name: str, model: torch.nn.Module, learning_rate: float, weight_decay: float, grad_accum_dtype: torch.dtype | None = None):
    """The reference's dispatch (:25-45) with its names; "adamw_torch" and "lion" are the fused HIP steps.
    `grad_accum_dtype=torch.float32`: fp32 gradient accumulation (the fused steps only)."""
    grouped_params = get_grouped_params(model, weight_decay)
    if grad_accum_dtype is not None and name not in ("adamw_torch", "lion"):
        raise ValueError(f'grad_accum_dtype needs a fused optimizer ("adamw_torch" or "lion"), not "{name}"')
    if name == "adamw_torch":
        return FusedAdamW(grouped_params, lr=learning_rate, grad_accum_dtype=grad_accum_dtype)
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
        return FusedLion(grouped_params, lr=learning_rate, grad_accum_dtype=grad_accum_dtype)
    raise ValueError(f"Unknown optimizer: {name}")
