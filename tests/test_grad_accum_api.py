"""Host side of the fp32 gradient accumulation: argument validation of `prl_optim_grad_accumulate` (the C entry validates before
any device work), the ctypes mirror of `prl_accum_segment`, and the options of `finetune/optim.py` / `PipelineSpec` - everything
that is checkable without a GPU."""

import ctypes
import re
from pathlib import Path

import pytest
import torch

from pipelinerl_amd import _lib
from pipelinerl_amd.finetune.optim import FusedAdamW, FusedLion, get_optimizer

FAKE = 0x10000  # validation never dereferences a pointer


def _err(libprl):
    return libprl.prl_last_error().decode()


def _table(n, numel=100, dtype=_lib.PRL_DTYPE_BF16):
    t = (_lib.PrlAccumSegment * n)()
    for s in t:
        s.grad, s.acc, s.numel, s.grad_dtype, s.reserved = FAKE, FAKE, numel, dtype, 0
    return t


def test_grad_accumulate_argument_validation(libprl):
    for overwrite in (0, 1):
        assert libprl.prl_optim_grad_accumulate(None, -1, overwrite, None) == _lib.PRL_EINVAL and "negative" in _err(libprl)
        assert libprl.prl_optim_grad_accumulate(None, 2, overwrite, None) == _lib.PRL_EINVAL and "null segment table" in _err(libprl)
        t = _table(3)
        t[2].grad_dtype = 7
        assert libprl.prl_optim_grad_accumulate(t, 3, overwrite, None) == _lib.PRL_EINVAL
        assert "segment 2" in _err(libprl) and "grad_dtype" in _err(libprl)
        t = _table(3)
        t[1].numel = -4
        assert libprl.prl_optim_grad_accumulate(t, 3, overwrite, None) == _lib.PRL_EINVAL and "segment 1" in _err(libprl) and "numel" in _err(libprl)
        t = _table(3, dtype=_lib.PRL_DTYPE_F32)
        t[1].acc = None  # a live gradient without an accumulator
        assert libprl.prl_optim_grad_accumulate(t, 3, overwrite, None) == _lib.PRL_EINVAL and "segment 1" in _err(libprl) and "acc" in _err(libprl)
        # nothing to do is not an error and touches no device: an empty table, and segments that are skipped
        assert libprl.prl_optim_grad_accumulate(None, 0, overwrite, None) == 0
        assert libprl.prl_optim_grad_accumulate(_table(1), 0, overwrite, None) == 0
        t = _table(2)
        t[0].grad, t[0].acc = None, None  # no gradient: skipped, its accumulator may be absent
        t[1].numel, t[1].acc = 0, None
        assert libprl.prl_optim_grad_accumulate(t, 2, overwrite, None) == 0


def test_accum_segment_struct_matches_the_header():
    text = (Path(__file__).resolve().parent.parent / "include" / "prl.h").read_text()
    body = re.search(r"typedef struct prl_accum_segment \{(.*?)\} prl_accum_segment;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(const void\*|void\*|int64_t|int32_t)\s+(\w+)\s*;", body)
    ctype = {"const void*": ctypes.c_void_p, "void*": ctypes.c_void_p, "int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32}
    assert [(name, ctype[t]) for t, name in fields] == list(_lib.PrlAccumSegment._fields_)
    assert [name for _, name in fields] == ["grad", "acc", "numel", "grad_dtype", "reserved"]
    assert ctypes.sizeof(_lib.PrlAccumSegment) == 2 * 8 + 8 + 2 * 4
    assert _lib.PROTOTYPES["prl_optim_grad_accumulate"] == (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p])


@pytest.mark.parametrize("cls", [FusedAdamW, FusedLion])
def test_grad_accum_dtype_option(cls):
    p = [torch.nn.Parameter(torch.zeros(3))]
    assert cls(p, lr=1e-3).grad_accum_dtype is None
    assert cls(p, lr=1e-3, grad_accum_dtype=torch.float32).grad_accum_dtype is torch.float32
    for bad in (torch.bfloat16, torch.float16, torch.float64, "float32"):
        with pytest.raises(ValueError, match="grad_accum_dtype"):
            cls(p, lr=1e-3, grad_accum_dtype=bad)
    opt = cls(p, lr=1e-3, grad_accum_dtype=torch.float32)
    assert opt.state_dict()["state"] == {} and opt._acc_flat is None  # state and accumulators are lazy
    with pytest.raises(RuntimeError, match="grad_accum_dtype"):
        cls(p, lr=1e-3).accumulate_grads()
    opt.accumulate_grads()  # nothing to fold: an fp32 parameter without a gradient
    opt.reduce_accumulated()  # no process group: a no-op
    assert opt._acc_flat is None


def test_unfolded_gradient_and_cpu_parameters_fail_loudly():
    p = torch.nn.Parameter(torch.zeros(8, dtype=torch.bfloat16))
    opt = FusedAdamW([p], lr=1e-3, grad_accum_dtype=torch.float32)
    p.grad = torch.ones(8, dtype=torch.bfloat16)
    for call in (opt.step, lambda: opt.clip_and_step(1.0), lambda: opt.compute_grad_norm(1.0)):
        with pytest.raises(RuntimeError, match="accumulate_grads"):
            call()
    with pytest.raises((RuntimeError, ImportError), match="no CPU fallback"):
        opt.accumulate_grads()
    assert p.grad is not None and torch.all(p.detach() == 0), "nothing was folded or stepped on the way"


def test_get_optimizer_forwards_the_option_and_keeps_the_four_argument_form():
    model = torch.nn.Linear(4, 4)
    for name, cls in (("adamw_torch", FusedAdamW), ("lion", FusedLion)):
        plain = get_optimizer(name, model, 2e-5, 0.1)
        assert isinstance(plain, cls) and plain.grad_accum_dtype is None and plain.master_weights
        assert [g["weight_decay"] for g in plain.param_groups] == [0.1, 0.0] and all(g["lr"] == 2e-5 for g in plain.param_groups)
        assert get_optimizer(name, model, 2e-5, 0.1, grad_accum_dtype=torch.float32).grad_accum_dtype is torch.float32
        assert get_optimizer(name, model, 2e-5, 0.1, torch.float32).grad_accum_dtype is torch.float32
        with pytest.raises(ValueError, match="grad_accum_dtype"):
            get_optimizer(name, model, 2e-5, 0.1, grad_accum_dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="fused optimizer"):
        get_optimizer("adafactor", model, 1e-4, 0.0, grad_accum_dtype=torch.float32)


def test_pipeline_spec_grad_accum_fp32_needs_adamw_hip(tmp_path):
    from pipelinerl_amd.pipeline_run import PipelineSpec

    assert PipelineSpec(exp_path=str(tmp_path)).grad_accum_fp32 is False
    assert PipelineSpec(exp_path=str(tmp_path), optimizer="adamw_hip", grad_accum_fp32=True).grad_accum_fp32 is True
    for other in ("adamw", "sgd"):
        with pytest.raises(ValueError, match="adamw_hip"):
            PipelineSpec(exp_path=str(tmp_path), optimizer=other, grad_accum_fp32=True)
