"""Host side of pipelinerl_amd/finetune/optim.py and the argument validation of the prl_optim_* entry points - everything that
is checkable without a GPU (the C entries validate before any device work)."""

import ctypes

import pytest
import torch

from pipelinerl_amd import _lib
from pipelinerl_amd.finetune.optim import FusedAdamW, FusedLion, get_grouped_params, get_optimizer


class Toy(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.embed = torch.nn.Embedding(8, 4)
        self.LayerNorm = torch.nn.LayerNorm(4)  # LayerNorm.weight / LayerNorm.bias
        self.proj = torch.nn.Linear(4, 4)       # proj.weight / proj.bias
        self.norm = torch.nn.LayerNorm(4)       # norm.weight DOES decay under the reference's rule (only its bias matches)


def test_get_grouped_params_is_the_reference_rule():
    model = Toy()
    groups = get_grouped_params(model, 0.1)
    assert [set(g) for g in groups] == [{"params", "weight_decay"}] * 2
    assert groups[0]["weight_decay"] == 0.1 and groups[1]["weight_decay"] == 0.0
    names = {id(p): n for n, p in model.named_parameters()}
    assert [names[id(p)] for p in groups[0]["params"]] == ["embed.weight", "proj.weight", "norm.weight"]
    assert [names[id(p)] for p in groups[1]["params"]] == ["LayerNorm.weight", "LayerNorm.bias", "proj.bias", "norm.bias"]
    custom = get_grouped_params(model, 0.1, no_decay=["norm"])
    assert [names[id(p)] for p in custom[1]["params"]] == ["norm.weight", "norm.bias"]


def test_get_optimizer_dispatch():
    model = Toy()
    opt = get_optimizer("adamw_torch", model, 2e-5, 0.1)
    assert isinstance(opt, FusedAdamW) and isinstance(opt, torch.optim.Optimizer) and opt.master_weights
    assert [g["weight_decay"] for g in opt.param_groups] == [0.1, 0.0] and all(g["lr"] == 2e-5 and g["betas"] == (0.9, 0.999) for g in opt.param_groups)
    lion = get_optimizer("lion", model, 3e-6, 0.1)
    assert isinstance(lion, FusedLion) and all(g["lr"] == 3e-6 and g["betas"] == (0.9, 0.99) for g in lion.param_groups)
    ada = get_optimizer("adafactor", model, 1e-4, 0.0)
    assert type(ada).__name__ == "Adafactor" and ada.param_groups[0]["relative_step"] is False and ada.param_groups[0]["scale_parameter"] is False
    with pytest.raises(ImportError, match="deepspeed"):
        get_optimizer("cpuadam", model, 1e-4, 0.0)
    with pytest.raises(ValueError, match="Unknown optimizer: sgd"):
        get_optimizer("sgd", model, 1e-4, 0.0)


@pytest.mark.parametrize("cls", [FusedAdamW, FusedLion])
def test_constructor_validation(cls):
    p = [torch.nn.Parameter(torch.zeros(3))]
    with pytest.raises(ValueError, match="learning rate"):
        cls(p, lr=-1.0)
    for betas in ((1.0, 0.9), (-0.1, 0.9)):
        with pytest.raises(ValueError, match="index 0"):
            cls(p, lr=1e-3, betas=betas)
    for betas in ((0.9, 1.0), (0.9, -0.5)):
        with pytest.raises(ValueError, match="index 1"):
            cls(p, lr=1e-3, betas=betas)
    opt = cls(p, lr=1e-3)
    assert opt.state_dict()["state"] == {}  # state is lazy


@pytest.mark.parametrize("cls", [FusedAdamW, FusedLion])
def test_cpu_parameters_fail_loudly(cls):
    model = Toy()
    opt = cls(model.parameters(), lr=1e-3)
    before = [p.detach().clone() for p in model.parameters()]
    model.proj(torch.ones(1, 4)).sum().backward()
    for call in (opt.step, lambda: opt.clip_and_step(1.0), lambda: opt.compute_grad_norm(1.0)):
        with pytest.raises((RuntimeError, ImportError), match="no CPU fallback"):
            call()
    assert all(torch.equal(a, b) for a, b in zip(before, model.parameters())), "no silent torch path"


def _segments(n):
    return (_lib.PrlOptimSegment * n)()


FAKE = 0x10000  # validation never dereferences a pointer


def _fill(seg, numel=100, grad_dtype=0, param_dtype=0):
    seg.param, seg.grad, seg.exp_avg, seg.exp_avg_sq, seg.master = FAKE, FAKE, FAKE, FAKE, None
    seg.numel, seg.step, seg.param_dtype, seg.grad_dtype, seg.lr, seg.weight_decay = numel, 1, param_dtype, grad_dtype, 1e-3, 0.0


def _err(libprl):
    return libprl.prl_last_error().decode()


def test_abi_argument_validation(libprl):
    need = ctypes.c_size_t(0)
    assert libprl.prl_optim_workspace_bytes(3, 1 << 20, None) == _lib.PRL_EINVAL and "null" in _err(libprl)
    assert libprl.prl_optim_workspace_bytes(-1, 0, ctypes.byref(need)) == _lib.PRL_EINVAL
    assert libprl.prl_optim_workspace_bytes(3, 1 << 20, ctypes.byref(need)) == 0 and need.value >= 8 * ((1 << 20) // 16384 + 3)

    calls = {
        "norm": lambda t, n: libprl.prl_optim_grad_norm(t, n, 1.0, FAKE, 1 << 20, FAKE, None),
        "adamw": lambda t, n: libprl.prl_optim_adamw_step(t, n, 0.9, 0.999, 1e-8, None, None),
        "lion": lambda t, n: libprl.prl_optim_lion_step(t, n, 0.9, 0.99, None, None),
    }
    for name, call in calls.items():
        assert call(None, 2) == _lib.PRL_EINVAL and "null segment table" in _err(libprl), name
        assert call(None, -1) == _lib.PRL_EINVAL, name
        t = _segments(3)
        for s in t:
            _fill(s)
        t[1].numel = -5
        assert call(t, 3) == _lib.PRL_EINVAL and "segment 1" in _err(libprl) and "numel" in _err(libprl), name
        _fill(t[1])
        t[2].grad_dtype = 7
        assert call(t, 3) == _lib.PRL_EINVAL and "segment 2" in _err(libprl) and "grad_dtype" in _err(libprl), name
        _fill(t[2])
        t[0].param_dtype = -1
        assert call(t, 3) == _lib.PRL_EINVAL and "segment 0" in _err(libprl) and "param_dtype" in _err(libprl), name

    t = _segments(2)
    for s in t:
        _fill(s, numel=40000)  # 3 chunks each: 48 bytes of partial records
    assert libprl.prl_optim_grad_norm(t, 2, 1.0, FAKE, 47, FAKE, None) == _lib.PRL_EINVAL and "workspace too small" in _err(libprl)
    assert libprl.prl_optim_grad_norm(t, 2, 1.0, None, 1 << 20, FAKE, None) == _lib.PRL_EINVAL and "workspace is null" in _err(libprl)
    assert libprl.prl_optim_grad_norm(t, 2, 1.0, FAKE, 1 << 20, None, None) == _lib.PRL_EINVAL and "norm_and_coef" in _err(libprl)

    # the step entries: state pointers, master/dtype pairing, step number, betas
    t = _segments(2)
    for s in t:
        _fill(s)
    t[1].exp_avg = None
    assert libprl.prl_optim_lion_step(t, 2, 0.9, 0.99, None, None) == _lib.PRL_EINVAL and "segment 1" in _err(libprl) and "exp_avg" in _err(libprl)
    _fill(t[1])
    t[1].exp_avg_sq = None
    assert libprl.prl_optim_adamw_step(t, 2, 0.9, 0.999, 1e-8, None, None) == _lib.PRL_EINVAL and "exp_avg_sq" in _err(libprl)
    _fill(t[1])
    t[0].master = FAKE  # fp32 parameter with a master copy
    assert libprl.prl_optim_adamw_step(t, 2, 0.9, 0.999, 1e-8, None, None) == _lib.PRL_EINVAL and "master" in _err(libprl)
    _fill(t[0])
    t[0].step = 0
    assert libprl.prl_optim_adamw_step(t, 2, 0.9, 0.999, 1e-8, None, None) == _lib.PRL_EINVAL and "step" in _err(libprl)
    _fill(t[0])
    assert libprl.prl_optim_adamw_step(t, 2, 1.0, 0.999, 1e-8, None, None) == _lib.PRL_EINVAL and "betas" in _err(libprl)
    assert libprl.prl_optim_lion_step(t, 2, 0.9, -0.1, None, None) == _lib.PRL_EINVAL and "betas" in _err(libprl)
    # nothing to do is not an error, and touches no device: zero segments, and segments without a gradient
    assert libprl.prl_optim_adamw_step(None, 0, 0.9, 0.999, 1e-8, None, None) == 0
    for s in t:
        s.grad = None
    assert libprl.prl_optim_adamw_step(t, 2, 0.9, 0.999, 1e-8, None, None) == 0
    assert libprl.prl_optim_lion_step(t, 2, 0.9, 0.99, None, None) == 0


def test_segment_struct_matches_the_header():
    import re
    from pathlib import Path

    text = (Path(__file__).resolve().parent.parent / "include" / "prl.h").read_text()
    body = re.search(r"typedef struct prl_optim_segment \{(.*?)\} prl_optim_segment;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(\w+)\s*;", body)
    assert fields == [f for f, _ in _lib.PrlOptimSegment._fields_]
    assert ctypes.sizeof(_lib.PrlOptimSegment) == 5 * 8 + 2 * 8 + 2 * 4 + 2 * 8


def test_pipeline_spec_accepts_adamw_hip(tmp_path):
    from pipelinerl_amd.pipeline_run import PipelineSpec

    assert PipelineSpec(exp_path=str(tmp_path)).optimizer == "adamw"
    assert PipelineSpec(exp_path=str(tmp_path), optimizer="adamw_hip").optimizer == "adamw_hip"
