"""`install_fused_attention` on a machine without a GPU: what it changes and what it leaves alone, the fallback that keeps packed
sequences and pad tokens apart on CPU tensors, and the agreement of include/prl.h, `_lib.PROTOTYPES` and the block sizes."""

import re
from pathlib import Path

import pytest
import torch

from pipelinerl_amd import _lib
from pipelinerl_amd import fused_attention as fa
from pipelinerl_amd.fused_attention import install_fused_attention, uninstall_fused_attention

transformers = pytest.importorskip("transformers")

ROOT = Path(__file__).resolve().parent.parent
ATTN_SYMBOLS = ("prl_attn_segments", "prl_attn_workspace_bytes", "prl_attn_varlen_fwd", "prl_attn_varlen_bwd")


def tiny_qwen2(seed=0, **kw):
    args = dict(vocab_size=512, hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1,
                max_position_embeddings=256, tie_word_embeddings=False, attn_implementation="sdpa")
    args.update(kw)
    cfg = transformers.Qwen2Config(**args)
    torch.manual_seed(seed)
    return transformers.Qwen2ForCausalLM(cfg).float().eval()


def test_install_switches_this_model_and_nothing_else():
    model, other = tiny_qwen2(), tiny_qwen2(seed=1)
    assert model.model.layers[0].self_attn.head_dim == 64
    before = {n: p for n, p in model.named_parameters()}
    modules = {n: m for n, m in model.named_modules()}
    assert install_fused_attention(model) is model
    assert model._prl_fused_attention == {"previous": "sdpa", "layers": 2, "skipped": []}
    assert model.config._attn_implementation == fa.NAME
    after = {n: p for n, p in model.named_parameters()}
    assert list(after) == list(before) and all(after[n] is before[n] for n in before)
    assert {n: m for n, m in model.named_modules()} == modules
    assert not any("forward" in vars(m) for m in model.modules())  # nothing is patched: the switch is the config's
    report = model._prl_fused_attention
    assert install_fused_attention(model) is model and model._prl_fused_attention is report  # idempotent
    # a second model in the same process that nobody installed it on still runs sdpa
    assert other.config._attn_implementation == "sdpa" and not hasattr(other, "_prl_fused_attention")
    fresh = tiny_qwen2(seed=2)
    assert fresh.config._attn_implementation == "sdpa"
    assert uninstall_fused_attention(model) is model
    assert model.config._attn_implementation == "sdpa" and not hasattr(model, "_prl_fused_attention")
    assert uninstall_fused_attention(model) is model  # (nothing to undo)


def test_composes_with_head_and_body_in_both_orders():
    from pipelinerl_amd.fused_body import install_fused_body
    from pipelinerl_amd.fused_head import install_fused_head

    names = [n for n, _ in tiny_qwen2().named_parameters()]
    a = install_fused_attention(install_fused_body(install_fused_head(tiny_qwen2())))
    b = install_fused_head(install_fused_body(install_fused_attention(tiny_qwen2())))
    c = install_fused_body(install_fused_attention(install_fused_head(tiny_qwen2())))
    for m in (a, b, c):
        assert m._prl_fused_head is not None and m._prl_fused_body["rmsnorm"] == 5 and m._prl_fused_body["swiglu"] == 2
        assert m._prl_fused_attention["layers"] == 2 and m.config._attn_implementation == fa.NAME
        assert [n for n, _ in m.named_parameters()] == names


def test_install_through_the_actor_critic_wrapper():
    class Wrapper(torch.nn.Module):  # the layout of AutoModelForCausalLMWithValueHead: `.pretrained_model` + `.value_head`
        def __init__(self):
            super().__init__()
            self.pretrained_model = tiny_qwen2()
            self.value_head = torch.nn.Linear(128, 1)

    w = install_fused_attention(Wrapper())
    assert w._prl_fused_attention["layers"] == 2 and w.pretrained_model.config._attn_implementation == fa.NAME
    assert install_fused_attention(w.pretrained_model)._prl_fused_attention is w._prl_fused_attention  # the same LM through its own handle
    uninstall_fused_attention(w)
    assert w.pretrained_model.config._attn_implementation == "sdpa" and not hasattr(w.pretrained_model, "_prl_fused_attention")


def test_layers_the_kernels_do_not_take_are_listed():
    model = install_fused_attention(tiny_qwen2(num_attention_heads=4, num_key_value_heads=2))  # head_dim 32
    rep = model._prl_fused_attention
    assert rep["layers"] == 0 and [n for n, _ in rep["skipped"]] == ["model.layers.0.self_attn", "model.layers.1.self_attn"]
    assert all("head_dim 32" in why for _, why in rep["skipped"])


def test_packed_equals_separate_on_the_cpu_fallback():
    """fp32 on the CPU: each sequence of a packed [1, 12] batch (5 + 7 tokens, attention_mask ones, per-sequence position_ids) gets
    the logits it gets alone."""
    model = tiny_qwen2()
    ids = torch.randint(0, 512, (1, 12), generator=torch.Generator().manual_seed(5))
    pos = torch.tensor([list(range(5)) + list(range(7))])
    ones = torch.ones(1, 12, dtype=torch.long)
    with torch.no_grad():
        alone = [model(input_ids=ids[:, s], attention_mask=ones[:, s], position_ids=pos[:, s]).logits for s in (slice(0, 5), slice(5, 12))]
        stock = model(input_ids=ids, attention_mask=ones, position_ids=pos).logits
        print(f"[attention] stock sdpa, packed against alone: second sequence off by {(stock[:, 5:] - alone[1]).abs().max().item():.3g} (max abs)")
        install_fused_attention(model)
        for mask in (ones, None):
            packed = model(input_ids=ids, attention_mask=mask, position_ids=pos).logits
            for got, want in ((packed[:, :5], alone[0]), (packed[:, 5:], alone[1])):
                err = (got - want).abs().max().item()
                print(f"[attention] installed, packed against alone (mask {'ones' if mask is not None else 'None'}): {err:.3g}")
                assert err <= 1e-5
    # and it trains: the fallback is differentiable
    model(input_ids=ids, attention_mask=ones, position_ids=pos).logits.square().mean().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())


def test_padded_batch_equals_the_stock_model_on_the_real_tokens():
    model = tiny_qwen2()
    ids = torch.randint(0, 512, (2, 8), generator=torch.Generator().manual_seed(6))
    mask = torch.tensor([[0, 0, 0, 1, 1, 1, 1, 1], [1, 1, 1, 1, 1, 1, 0, 0]])
    pos = (mask.cumsum(-1) - 1).clamp(min=0)
    with torch.no_grad():
        stock = model(input_ids=ids, attention_mask=mask, position_ids=pos).logits
        install_fused_attention(model)
        got = model(input_ids=ids, attention_mask=mask, position_ids=pos).logits
    real = mask.bool()
    err = (got[real] - stock[real]).abs().max().item()
    print(f"[attention] padded [2, 8] batch, installed against stock on the real tokens: {err:.3g}")
    assert err <= 1e-5
    assert torch.isfinite(got).all()  # a pad token attends to itself: no empty row


def test_kv_cache_call_raises_with_the_way_out():
    model = install_fused_attention(tiny_qwen2())
    ids = torch.randint(0, 512, (1, 5), generator=torch.Generator().manual_seed(7))
    with pytest.raises(NotImplementedError) as e:
        model.generate(ids, max_new_tokens=2, do_sample=False)
    assert "learner" in str(e.value) and "uninstall_fused_attention" in str(e.value)
    uninstall_fused_attention(model)
    assert model.generate(ids, max_new_tokens=2, do_sample=False).shape == (1, 7)


def test_segment_table_is_computed_once_per_forward():
    model = install_fused_attention(tiny_qwen2())
    calls = []
    real = fa.segments

    def counting(*a, **k):
        calls.append(1)
        return real(*a, **k)

    ids = torch.randint(0, 512, (1, 12), generator=torch.Generator().manual_seed(8))
    pos = torch.tensor([list(range(5)) + list(range(7))])
    fa.segments = counting
    try:
        with torch.no_grad():
            model(input_ids=ids, attention_mask=torch.ones(1, 12, dtype=torch.long), position_ids=pos)
            assert len(calls) == 1  # two layers, one table
            pos[0, 5] = 5  # the same tensor, written in place: its version moved
            model(input_ids=ids, attention_mask=torch.ones(1, 12, dtype=torch.long), position_ids=pos)
            assert len(calls) == 2
    finally:
        fa.segments = real
    assert len(fa._seg_cache) <= fa._CACHE_ENTRIES


def test_varlen_attention_raises_on_cpu_tensors():
    q = torch.zeros(4, 2, 64, dtype=torch.bfloat16)
    ss, se = fa.segments(shape=(1, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fa.varlen_attention(q, q[:, :1], q[:, :1], ss, se, 0.125)


def test_header_prototypes_and_block_sizes_agree():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "prl.h").read_text(), flags=re.S)
    for sym in ATTN_SYMBOLS:
        m = re.search(rf"\bint\s+{sym}\s*\(([^;{{]*?)\)\s*;", text, flags=re.S)
        assert m is not None, f"{sym} is not declared in include/prl.h"
        n = len([p for p in m.group(1).split(",") if p.strip()])
        assert sym in _lib.PROTOTYPES and len(_lib.PROTOTYPES[sym][1]) == n, sym
    src = (ROOT / "pipelinerl_amd" / "csrc" / "prl_attention.hip").read_text()
    sizes = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define PRL_ATTN_(BQ|BK) (\d+)", src)}
    assert sizes == {"BQ": fa.BQ, "BK": fa.BK}
    assert "prl_attention.hip" in __import__("pipelinerl_amd.build", fromlist=["SOURCES"]).SOURCES
