"""`install_fused_body` on a machine without a GPU: what it patches and what it leaves alone, the CPU fallback of a patched
forward, and the agreement of include/prl.h, `_lib.PROTOTYPES` and the geometry constants for the fused body entry points."""

import copy
import re
from pathlib import Path

import pytest
import torch

from pipelinerl_amd import _lib
from pipelinerl_amd.fused_body import MLP_CLASSES, RMSNORM_CLASSES, install_fused_body

transformers = pytest.importorskip("transformers")

ROOT = Path(__file__).resolve().parent.parent
BODY_SYMBOLS = ("prl_rmsnorm_workspace_bytes", "prl_rmsnorm_fwd", "prl_rmsnorm_bwd", "prl_swiglu_fwd", "prl_swiglu_bwd")


def tiny_qwen2(hidden_act="silu", seed=0):
    cfg = transformers.Qwen2Config(vocab_size=512, hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4,
                                   num_key_value_heads=2, max_position_embeddings=256, tie_word_embeddings=False, hidden_act=hidden_act,
                                   attn_implementation="eager")
    torch.manual_seed(seed)
    return transformers.Qwen2ForCausalLM(cfg).float()


def test_install_patches_forwards_and_nothing_else():
    model = tiny_qwen2()
    before = {n: p for n, p in model.named_parameters()}
    keys = list(model.state_dict().keys())
    modules = {n: m for n, m in model.named_modules()}
    assert install_fused_body(model) is model
    assert model._prl_fused_body == {"rmsnorm": 5, "swiglu": 2, "skipped": []}
    after = {n: p for n, p in model.named_parameters()}
    assert list(after) == list(before) and all(after[n] is before[n] for n in before)
    assert list(model.state_dict().keys()) == keys
    assert {n: m for n, m in model.named_modules()} == modules  # the same module objects under the same names
    patched = [n for n, m in model.named_modules() if "forward" in vars(m)]
    assert len(patched) == 7 and all(type(modules[n]).__name__ in RMSNORM_CLASSES + MLP_CLASSES for n in patched)
    # idempotent: a second call wraps nothing twice
    forwards = {n: vars(modules[n])["forward"] for n in patched}
    report = model._prl_fused_body
    assert install_fused_body(model) is model and model._prl_fused_body is report
    assert all(vars(modules[n])["forward"] is forwards[n] for n in patched)
    copy.deepcopy(model.state_dict())  # (still serialisable)


def test_cpu_tensors_take_the_original_forward_bit_for_bit():
    stock = tiny_qwen2()
    fused = install_fused_body(copy.deepcopy(stock))
    ids = torch.randint(0, 512, (2, 17), generator=torch.Generator().manual_seed(3))
    a = stock(input_ids=ids).logits
    b = fused(input_ids=ids).logits
    assert torch.equal(a, b)
    a.square().mean().backward()
    b.square().mean().backward()
    for (n, p), (_, q) in zip(stock.named_parameters(), fused.named_parameters()):
        assert torch.equal(p.grad, q.grad), n


def test_a_model_with_another_activation_is_skipped_with_the_reason():
    model = install_fused_body(tiny_qwen2(hidden_act="gelu"))
    rep = model._prl_fused_body
    assert rep["rmsnorm"] == 5 and rep["swiglu"] == 0
    assert [n for n, _ in rep["skipped"]] == ["model.layers.0.mlp", "model.layers.1.mlp"]
    assert all("hidden_act" in why and "gelu" in why for _, why in rep["skipped"])
    assert not any("forward" in vars(m) for n, m in model.named_modules() if n.endswith(".mlp"))


def test_switches_and_the_order_with_the_fused_head():
    from pipelinerl_amd.fused_head import install_fused_head

    only_norm = install_fused_body(tiny_qwen2(), swiglu=False)
    assert only_norm._prl_fused_body["rmsnorm"] == 5 and only_norm._prl_fused_body["swiglu"] == 0
    assert all(why == "swiglu=False" for _, why in only_norm._prl_fused_body["skipped"]) and len(only_norm._prl_fused_body["skipped"]) == 2
    a = install_fused_body(install_fused_head(tiny_qwen2()))
    b = install_fused_head(install_fused_body(tiny_qwen2()))
    for m in (a, b):
        assert m._prl_fused_head is not None and m._prl_fused_body["rmsnorm"] == 5 and m._prl_fused_body["swiglu"] == 2
        assert [n for n, _ in m.named_parameters()] == [n for n, _ in tiny_qwen2().named_parameters()]


def test_install_through_the_actor_critic_wrapper():
    class Wrapper(torch.nn.Module):  # the layout of AutoModelForCausalLMWithValueHead: `.pretrained_model` + `.value_head`
        def __init__(self):
            super().__init__()
            self.pretrained_model = tiny_qwen2()
            self.value_head = torch.nn.Linear(64, 1)

    w = install_fused_body(Wrapper())
    assert w._prl_fused_body["rmsnorm"] == 5 and w._prl_fused_body["swiglu"] == 2
    assert "forward" in vars(w.pretrained_model.model.norm)


def test_header_and_prototypes_list_the_body_entry_points():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "prl.h").read_text(), flags=re.S)
    for sym in BODY_SYMBOLS:
        m = re.search(rf"\bint\s+{sym}\s*\(([^;{{]*?)\)\s*;", text, flags=re.S)
        assert m is not None, f"{sym} is not declared in include/prl.h"
        n = len([p for p in m.group(1).split(",") if p.strip()])
        assert sym in _lib.PROTOTYPES and len(_lib.PROTOTYPES[sym][1]) == n, sym
    assert int(re.search(r"#define PRL_ABI_VERSION (\d+)", text).group(1)) == _lib.PRL_ABI_VERSION == 19  # additive: the version stays


def test_geometry_constants_equal_the_header():
    text = (ROOT / "pipelinerl_amd" / "csrc" / "prl_body_math.h").read_text()
    header = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define PRL_BODY_(\w+) (\d+)", text)}
    assert header == _lib.BODY_GEOMETRY


def test_a_stale_library_is_reported_as_one(tmp_path, libprl):
    """A shared object with the right version number but without the new symbols raises the 'rebuild' ImportError."""
    import subprocess
    import sys

    src = tmp_path / "stale.c"
    src.write_text("int prl_abi_version(void) { return 19; }\n")
    so = tmp_path / "libprl.so"
    subprocess.check_call(["gcc", "-shared", "-fPIC", "-o", str(so), str(src)])
    code = ("import os, sys; sys.path.insert(0, %r); os.environ['PRL_LIB'] = %r\n"
            "from pipelinerl_amd import _lib\n"
            "try:\n    _lib.load()\nexcept ImportError as e:\n    assert 'rebuild' in str(e), e\n    print('IMPORT_ERROR')\n") % (str(ROOT), str(so))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "IMPORT_ERROR" in out.stdout, out.stdout + out.stderr[-2000:]
