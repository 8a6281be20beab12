"""Host side of `FusedAdafactor` / `get_optimizer("adafactor_hip")` and the argument validation of the prl_adafactor_* entry points:
everything that is checkable without a GPU (the C entries validate before any device work)."""

import ctypes
import re
from pathlib import Path

import pytest
import torch

from pipelinerl_amd import _lib
from pipelinerl_amd.finetune.optim import FusedAdafactor, get_optimizer

from test_optim_api import Toy

FAKE = 0x10000  # validation never dereferences a pointer


def test_get_optimizer_returns_the_fused_step_with_the_references_rule():
    model = Toy()
    opt = get_optimizer("adafactor_hip", model, 1e-4, 0.1)
    assert isinstance(opt, FusedAdafactor) and isinstance(opt, torch.optim.Optimizer) and opt.master_weights and opt.grad_accum_dtype is None
    assert [g["weight_decay"] for g in opt.param_groups] == [0.1, 0.0]
    ref = get_optimizer("adafactor", model, 1e-4, 0.1)
    assert type(ref).__name__ == "Adafactor"
    for g, r in zip(opt.param_groups, ref.param_groups):  # the reference's hyper-parameters, under transformers' keys
        assert {k: v for k, v in g.items() if k != "params"} == {k: v for k, v in r.items() if k != "params"}
        assert [id(p) for p in g["params"]] == [id(p) for p in r["params"]]
    assert all(hasattr(opt, m) for m in ("accumulate_grads", "reduce_accumulated", "compute_grad_norm", "clip_and_step", "step", "zero_grad"))
    acc = get_optimizer("adafactor_hip", model, 1e-4, 0.1, grad_accum_dtype=torch.float32)
    assert isinstance(acc, FusedAdafactor) and acc.grad_accum_dtype == torch.float32
    assert opt.state_dict()["state"] == {}  # state is lazy


def test_constructor_rejects_what_is_not_built():
    p = [torch.nn.Parameter(torch.zeros(3, 4))]
    for kw, name in (({"beta1": 0.9}, "beta1"), ({"relative_step": True}, "relative_step"), ({"scale_parameter": True}, "scale_parameter")):
        with pytest.raises(ValueError, match=name):
            FusedAdafactor(p, lr=1e-3, **kw)
    with pytest.raises(ValueError, match="not built for Adafactor"):
        FusedAdafactor(p, lr=1e-3, shard=(0, 2))
    with pytest.raises(ValueError, match="not built for Adafactor"):
        FusedAdafactor(p, lr=1e-3, shard_group=object())
    with pytest.raises(ValueError, match="not built for Adafactor"):
        get_optimizer("adafactor_hip", Toy(), 1e-4, 0.0, shard=(0, 2))
    for bad in (torch.bfloat16, torch.float16, torch.float64):
        with pytest.raises(ValueError, match="grad_accum_dtype"):
            FusedAdafactor(p, lr=1e-3, grad_accum_dtype=bad)
    with pytest.raises(ValueError, match="learning rate"):
        FusedAdafactor(p, lr=-1.0)
    with pytest.raises(ValueError, match="clip_threshold"):
        FusedAdafactor(p, lr=1e-3, clip_threshold=0.0)
    with pytest.raises(ValueError, match="decay_rate"):
        FusedAdafactor(p, lr=1e-3, decay_rate=0.5)


def test_state_shapes_follow_transformers():
    opt = FusedAdafactor([torch.nn.Parameter(torch.zeros(2, 3, 5)), torch.nn.Parameter(torch.zeros(7))], lr=1e-3)
    a, b = opt.param_groups[0]["params"]
    assert opt._keys_of(a) == ("exp_avg_sq_row", "exp_avg_sq_col") and opt._keys_of(b) == ("exp_avg_sq",)
    assert opt._state_shape(a, "exp_avg_sq_row") == (2, 3) and opt._state_shape(a, "exp_avg_sq_col") == (2, 5) and opt._state_shape(b, "exp_avg_sq") == (7,)
    bf = torch.nn.Parameter(torch.zeros(3, 5, dtype=torch.bfloat16))
    assert FusedAdafactor([bf], lr=1e-3)._keys_of(bf)[-1] == "master" and FusedAdafactor([bf], lr=1e-3, master_weights=False)._keys_of(bf)[-1] != "master"


def test_cpu_parameters_fail_loudly():
    model = Toy()
    opt = FusedAdafactor(model.parameters(), lr=1e-3)
    before = [p.detach().clone() for p in model.parameters()]
    model.proj(torch.ones(1, 4)).sum().backward()
    for call in (opt.step, lambda: opt.clip_and_step(1.0), lambda: opt.compute_grad_norm(1.0)):
        with pytest.raises((RuntimeError, ImportError), match="no CPU fallback"):
            call()
    assert all(torch.equal(a, b) for a, b in zip(before, model.parameters())), "no silent torch path"


def _fill(seg, batch=1, rows=10, cols=10, factored=True, grad_dtype=0, param_dtype=0):
    seg.param, seg.grad, seg.master = FAKE, FAKE, None
    seg.row, seg.col, seg.v = (FAKE, FAKE, None) if factored else (None, None, FAKE)
    seg.batch, seg.rows, seg.cols, seg.step = batch, rows, cols, 1
    seg.param_dtype, seg.grad_dtype, seg.lr, seg.weight_decay = param_dtype, grad_dtype, 1e-3, 0.0


def _err(libprl):
    return libprl.prl_last_error().decode()


def test_abi_argument_validation(libprl):
    EINVAL = _lib.PRL_EINVAL

    def step(t, n, ws=FAKE, ws_bytes=1 << 30, eps1=1e-30, clip=1.0, decay=-0.8):
        return libprl.prl_adafactor_step(t, n, eps1, clip, decay, None, ws, ws_bytes, None)

    need = ctypes.c_size_t(0)
    assert step(None, 2) == EINVAL and "null segment table" in _err(libprl)
    assert step(None, -1) == EINVAL
    assert libprl.prl_adafactor_workspace_bytes(None, 2, ctypes.byref(need)) == EINVAL and "null segment table" in _err(libprl)
    t = (_lib.PrlAdafactorSegment * 3)()
    for s in t:
        _fill(s)
    assert libprl.prl_adafactor_workspace_bytes(t, 3, None) == EINVAL and "null" in _err(libprl)
    t[1].rows = -5
    assert step(t, 3) == EINVAL and "segment 1" in _err(libprl) and "negative" in _err(libprl)
    _fill(t[1], batch=1 << 31, rows=1 << 31, cols=1 << 31)
    assert step(t, 3) == EINVAL and "segment 1" in _err(libprl) and "too many" in _err(libprl)
    _fill(t[1])
    t[2].grad_dtype = 7
    assert step(t, 3) == EINVAL and "segment 2" in _err(libprl) and "grad_dtype" in _err(libprl)
    _fill(t[2])
    t[0].param_dtype = -1
    assert step(t, 3) == EINVAL and "segment 0" in _err(libprl) and "param_dtype" in _err(libprl)
    _fill(t[0])
    t[0].master = FAKE  # fp32 parameter with a master copy
    assert step(t, 3) == EINVAL and "segment 0" in _err(libprl) and "master" in _err(libprl)
    _fill(t[0])
    t[2].step = 0
    assert step(t, 3) == EINVAL and "segment 2" in _err(libprl) and "step" in _err(libprl)
    _fill(t[2])
    for missing in ("row", "col"):
        setattr(t[1], missing, None)
        assert step(t, 3) == EINVAL and "segment 1" in _err(libprl) and "row and col" in _err(libprl)
        _fill(t[1])
    _fill(t[1], rows=3, factored=False)  # an unfactored segment is one run of elements
    assert step(t, 3) == EINVAL and "segment 1" in _err(libprl) and "unfactored" in _err(libprl)
    _fill(t[1])
    assert step(t, 3, clip=0.0) == EINVAL and "clip_threshold" in _err(libprl)
    assert step(t, 3, eps1=-1.0) == EINVAL and "eps1" in _err(libprl)
    assert step(t, 3, decay=0.5) == EINVAL and "decay_rate" in _err(libprl)
    # the workspace: sized by the library, checked before any launch
    assert libprl.prl_adafactor_workspace_bytes(t, 3, ctypes.byref(need)) == 0 and need.value > 0 and need.value % 16 == 0
    assert step(t, 3, ws_bytes=need.value - 1) == EINVAL and "workspace too small" in _err(libprl)
    assert step(t, 3, ws=None) == EINVAL and "workspace is null" in _err(libprl)
    assert step(t, 3, ws=FAKE + 4) == EINVAL and "aligned" in _err(libprl)
    # nothing to do is not an error, and touches no device: zero segments, segments without a gradient or without elements
    assert step(None, 0) == 0
    assert libprl.prl_adafactor_workspace_bytes(None, 0, ctypes.byref(need)) == 0 and need.value == 0
    for s in t:
        s.grad = None
    assert step(t, 3, ws=None, ws_bytes=0) == 0
    for s in t:
        _fill(s, cols=0)
    assert step(t, 3, ws=None, ws_bytes=0) == 0
    geo = [ctypes.c_int64() for _ in range(4)]
    assert libprl.prl_adafactor_geometry(*[ctypes.byref(g) for g in geo]) == 0 and all(g.value > 0 for g in geo)
    assert libprl.prl_adafactor_geometry(None, None, None, None) == EINVAL


def test_segment_struct_matches_the_header():
    text = (Path(__file__).resolve().parent.parent / "include" / "prl.h").read_text()
    body = re.search(r"typedef struct prl_adafactor_segment \{(.*?)\} prl_adafactor_segment;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(\w+)\s*;", body)
    assert fields == [f for f, _ in _lib.PrlAdafactorSegment._fields_]
    assert fields == ["param", "grad", "master", "row", "col", "v", "batch", "rows", "cols", "step", "param_dtype", "grad_dtype", "lr", "weight_decay"]
    assert ctypes.sizeof(_lib.PrlAdafactorSegment) == 6 * 8 + 4 * 8 + 2 * 4 + 2 * 8


def test_pipeline_spec_accepts_adafactor_hip(tmp_path):
    from pipelinerl_amd.pipeline_run import PipelineSpec

    assert PipelineSpec(exp_path=str(tmp_path), optimizer="adafactor_hip").optimizer == "adafactor_hip"
    assert PipelineSpec(exp_path=str(tmp_path), optimizer="adafactor_hip", grad_accum_fp32=True).grad_accum_fp32
    with pytest.raises(ValueError, match="adamw_hip"):
        PipelineSpec(exp_path=str(tmp_path), optimizer="adamw", grad_accum_fp32=True)
    with pytest.raises(ValueError, match="shard_optimizer_state"):
        PipelineSpec(exp_path=str(tmp_path), optimizer="adafactor_hip", shard_optimizer_state=True)
