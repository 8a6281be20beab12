"""Host side of the compact-state options of `FusedAdamW` / `FusedLion` (`state_dtype`, `param_rounding`, `seed`) and the argument
validation of `prl_optim_adamw_step_compact` / `prl_optim_lion_step_compact` - everything that is checkable without a GPU (the C
entries validate before any device work)."""

import ctypes
import re
from pathlib import Path

import pytest
import torch

from pipelinerl_amd import _lib
from pipelinerl_amd.finetune.optim import FusedAdafactor, FusedAdamW, FusedLion, get_optimizer


class Toy(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.embed = torch.nn.Embedding(8, 4)
        self.proj = torch.nn.Linear(4, 4)


@pytest.mark.parametrize("cls", [FusedAdamW, FusedLion])
def test_constructor_options(cls):
    p = [torch.nn.Parameter(torch.zeros(3))]
    for bad in (torch.float16, torch.float64, "bf16"):
        with pytest.raises(ValueError, match="state_dtype"):
            cls(p, state_dtype=bad)
    for bad in ("random", "", None, "Stochastic"):
        with pytest.raises(ValueError, match="param_rounding"):
            cls(p, param_rounding=bad)
    for bad in (-1, 1 << 64, 1.5, "7", True):
        with pytest.raises(ValueError, match="seed"):
            cls(p, seed=bad)
    plain = cls(p)
    assert plain.state_dtype == torch.float32 and plain.param_rounding == "nearest" and not plain._compact
    assert plain._segment_type is _lib.PrlOptimSegment, "the defaults keep the existing table and entry points"
    assert all(g["seed"] == 0 for g in plain.param_groups) and plain.defaults["seed"] == 0
    assert not cls(p, state_dtype=torch.float32, param_rounding="nearest", seed=9)._compact, "a seed alone changes nothing"
    for kw in (dict(state_dtype=torch.bfloat16), dict(param_rounding="stochastic"), dict(state_dtype=torch.bfloat16, param_rounding="stochastic", seed=(1 << 64) - 1)):
        opt = cls(p, **kw)
        assert opt._compact and opt._segment_type is _lib.PrlOptimCompactSegment
        assert opt.state_dtype == kw.get("state_dtype", torch.float32) and opt.param_rounding == kw.get("param_rounding", "nearest")
        assert all(g["seed"] == kw.get("seed", 0) for g in opt.param_groups)
        assert opt.state_dict()["param_groups"][0]["seed"] == kw.get("seed", 0), "the seed travels with state_dict()"
        assert opt.state_dict()["state"] == {}  # state is lazy
    # allowed, and documented as having no effect on parameters that have a master copy
    assert cls(p, param_rounding="stochastic", master_weights=True).master_weights


def test_seed_survives_a_state_dict_without_one():
    p = [torch.nn.Parameter(torch.zeros(3))]
    saved = torch.optim.AdamW([torch.nn.Parameter(torch.zeros(3))], lr=1e-3).state_dict()
    assert "seed" not in saved["param_groups"][0]
    opt = FusedAdamW(p, state_dtype=torch.bfloat16, seed=77)
    opt.load_state_dict(saved)
    assert opt.param_groups[0]["seed"] == 77
    other = FusedAdamW([torch.nn.Parameter(torch.zeros(3))], state_dtype=torch.bfloat16, seed=5)
    other.load_state_dict(FusedAdamW(p, state_dtype=torch.bfloat16, seed=123).state_dict())
    assert other.param_groups[0]["seed"] == 123, "a resumed run takes the saved seed"


def test_get_optimizer_plumbing_and_refusals():
    model = Toy()
    for name, cls in (("adamw_torch", FusedAdamW), ("lion", FusedLion)):
        opt = get_optimizer(name, model, 1e-4, 0.1, state_dtype=torch.bfloat16, param_rounding="stochastic", seed=42)
        assert isinstance(opt, cls) and opt.state_dtype == torch.bfloat16 and opt.param_rounding == "stochastic"
        assert [g["seed"] for g in opt.param_groups] == [42, 42] and [g["weight_decay"] for g in opt.param_groups] == [0.1, 0.0]
        plain = get_optimizer(name, model, 1e-4, 0.1)
        assert not plain._compact and plain.state_dtype == torch.float32 and plain.master_weights
        assert not get_optimizer(name, model, 1e-4, 0.1, state_dtype=None, param_rounding="nearest", seed=0)._compact
        with pytest.raises(ValueError, match="state_dtype"):
            get_optimizer(name, model, 1e-4, 0.1, state_dtype=torch.float16)
    for name in ("adafactor", "adafactor_hip", "cpuadam", "sgd"):
        for kw in (dict(state_dtype=torch.bfloat16), dict(param_rounding="stochastic"), dict(seed=1)):
            with pytest.raises(ValueError, match="compact optimizer state"):
                get_optimizer(name, model, 1e-4, 0.0, **kw)
    for kw in (dict(state_dtype=torch.bfloat16), dict(param_rounding="stochastic"), dict(seed=1)):
        with pytest.raises(ValueError, match="not built for Adafactor"):
            FusedAdafactor(model.parameters(), **kw)
    assert isinstance(get_optimizer("adafactor_hip", model, 1e-4, 0.0, state_dtype=torch.float32), FusedAdafactor)


def test_compact_segment_struct_matches_the_header():
    text = (Path(__file__).resolve().parent.parent / "include" / "prl.h").read_text()
    body = re.search(r"typedef struct prl_optim_compact_segment \{(.*?)\} prl_optim_compact_segment;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(\w+)\s*;", body)
    assert fields == [f for f, _ in _lib.PrlOptimCompactSegment._fields_]
    plain = [f for f, _ in _lib.PrlOptimSegment._fields_]
    assert fields[:len(plain)] == plain and fields[len(plain):] == ["state_dtype", "param_rounding", "elem_offset", "ordinal"]
    assert ctypes.sizeof(_lib.PrlOptimCompactSegment) == ctypes.sizeof(_lib.PrlOptimSegment) + 2 * 4 + 2 * 8
    for name in ("param", "numel", "step", "lr", "weight_decay"):  # the common prefix has the same layout
        assert getattr(_lib.PrlOptimCompactSegment, name).offset == getattr(_lib.PrlOptimSegment, name).offset
    assert int(re.search(r"#define PRL_ROUND_STOCHASTIC (\d+)", text).group(1)) == _lib.PRL_ROUND_STOCHASTIC == 1
    assert int(re.search(r"#define PRL_ROUND_NEAREST (\d+)", text).group(1)) == _lib.PRL_ROUND_NEAREST == 0


FAKE = 0x10000  # validation never dereferences a pointer


def _fill(seg, numel=100, param_dtype=_lib.PRL_DTYPE_BF16, state_dtype=_lib.PRL_DTYPE_BF16, rounding=_lib.PRL_ROUND_STOCHASTIC):
    seg.param, seg.grad, seg.exp_avg, seg.exp_avg_sq, seg.master = FAKE, FAKE, FAKE, FAKE, None
    seg.numel, seg.step, seg.param_dtype, seg.grad_dtype, seg.lr, seg.weight_decay = numel, 1, param_dtype, _lib.PRL_DTYPE_BF16, 1e-3, 0.0
    seg.state_dtype, seg.param_rounding, seg.elem_offset, seg.ordinal = state_dtype, rounding, 0, 0


def _err(libprl):
    return libprl.prl_last_error().decode()


def test_compact_abi_argument_validation(libprl):
    calls = {
        "adamw": lambda t, n: libprl.prl_optim_adamw_step_compact(t, n, 0.9, 0.999, 1e-8, 7, None, None),
        "lion": lambda t, n: libprl.prl_optim_lion_step_compact(t, n, 0.9, 0.99, 7, None, None),
    }
    bad_fields = [  # (segment, field, value, words the message carries)
        (1, "numel", -5, ("numel",)),
        (2, "grad_dtype", 7, ("grad_dtype",)),
        (0, "param_dtype", -1, ("param_dtype",)),
        (1, "state_dtype", 2, ("state_dtype",)),
        (2, "state_dtype", -1, ("state_dtype",)),
        (0, "param_rounding", 2, ("param_rounding",)),
        (1, "param_rounding", -1, ("param_rounding",)),
        (2, "master", FAKE, ("stochastic", "master")),
        (0, "elem_offset", -4, ("negative elem_offset",)),
        (1, "elem_offset", 6, ("elem_offset", "multiple of 4")),
        (2, "ordinal", -1, ("ordinal",)),
        (0, "ordinal", 1 << 32, ("ordinal",)),
        (1, "exp_avg", None, ("exp_avg",)),
        (2, "step", 0, ("step",)),
    ]
    for name, call in calls.items():
        assert call(None, 2) == _lib.PRL_EINVAL and "null segment table" in _err(libprl), name
        assert call(None, -1) == _lib.PRL_EINVAL, name
        for index, field, value, words in bad_fields:  # every bad field is named together with its segment
            t = (_lib.PrlOptimCompactSegment * 3)()
            for s in t:
                _fill(s)
            setattr(t[index], field, value)
            assert call(t, 3) == _lib.PRL_EINVAL, (name, field)
            assert f"segment {index}" in _err(libprl) and all(w in _err(libprl) for w in words), (name, field, _err(libprl))
    t = (_lib.PrlOptimCompactSegment * 2)()
    for s in t:
        _fill(s)
    t[1].exp_avg_sq = None
    assert libprl.prl_optim_adamw_step_compact(t, 2, 0.9, 0.999, 1e-8, 0, None, None) == _lib.PRL_EINVAL and "segment 1" in _err(libprl) and "exp_avg_sq" in _err(libprl)
    _fill(t[1])
    t[0].param_dtype, t[0].param_rounding, t[0].master = _lib.PRL_DTYPE_F32, _lib.PRL_ROUND_NEAREST, FAKE  # fp32 parameter with a master copy
    assert libprl.prl_optim_adamw_step_compact(t, 2, 0.9, 0.999, 1e-8, 0, None, None) == _lib.PRL_EINVAL and "master" in _err(libprl)
    _fill(t[0])
    assert libprl.prl_optim_adamw_step_compact(t, 2, 1.0, 0.999, 1e-8, 0, None, None) == _lib.PRL_EINVAL and "betas" in _err(libprl)
    assert libprl.prl_optim_adamw_step_compact(t, 2, 0.9, 0.999, -1.0, 0, None, None) == _lib.PRL_EINVAL and "eps" in _err(libprl)
    assert libprl.prl_optim_lion_step_compact(t, 2, 0.9, -0.1, 0, None, None) == _lib.PRL_EINVAL and "betas" in _err(libprl)
    # nothing to do is not an error, and touches no device: zero segments, and segments without a gradient
    assert libprl.prl_optim_adamw_step_compact(None, 0, 0.9, 0.999, 1e-8, 0, None, None) == 0
    for s in t:
        s.grad = None
    assert libprl.prl_optim_adamw_step_compact(t, 2, 0.9, 0.999, 1e-8, (1 << 64) - 1, None, None) == 0
    assert libprl.prl_optim_lion_step_compact(t, 2, 0.9, 0.99, (1 << 64) - 1, None, None) == 0
