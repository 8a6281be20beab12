"""`install_fused_attention` on a tiny bf16 Qwen2ForCausalLM on the GPU: loss and every parameter gradient of the installed
model on a PACKED batch of three sequences against an fp64 copy of the model run on each sequence alone and summed.  Per tensor,
with err = max |got - want| / max |want|, the installed model may be at most 4 x as far from fp64 as the stock bf16 model run
sequence by sequence is (the project's standing margin).  Composed with `install_fused_head` and `install_fused_body`,
`rl_step_fused_head` runs and its loss meets the same criterion against `rl_step` on the model with the attention alone."""

import copy

import pytest
import torch
import torch.nn.functional as F

from pipelinerl_amd import fused_attention as fa
from pipelinerl_amd.fused_attention import install_fused_attention
from pipelinerl_amd.fused_body import RMSNORM_CLASSES, install_fused_body

transformers = pytest.importorskip("transformers")
pytestmark = pytest.mark.gpu

V, LENGTHS, PROMPT = 512, (17, 70, 41), 4  # 128 tokens: the second sequence crosses a block edge, the third starts inside a block
MARGIN = 4.0


def tiny(kind="qwen2"):
    args = dict(vocab_size=V, hidden_size=128, intermediate_size=256, num_hidden_layers=2, max_position_embeddings=256, tie_word_embeddings=False,
                attn_implementation="sdpa")
    torch.manual_seed(0)
    if kind == "qwen2":  # head_dim 64, two query heads on one KV head
        return transformers.Qwen2ForCausalLM(transformers.Qwen2Config(num_attention_heads=2, num_key_value_heads=1, **args)).to(torch.bfloat16)
    return transformers.LlamaForCausalLM(transformers.LlamaConfig(num_attention_heads=2, num_key_value_heads=2, **args)).to(torch.bfloat16)


def fp64_copy(model):
    """The model in fp64 on the CPU (transformers' RMSNorm computes in fp32 whatever it is given: here its formula runs in fp64)."""
    wit = copy.deepcopy(model).double().cpu()
    for m in wit.modules():
        if type(m).__name__ in RMSNORM_CLASSES:
            m.forward = lambda h, m=m: m.weight * (h * torch.rsqrt(h.pow(2).mean(-1, keepdim=True) + m.variance_epsilon))
    return wit


def sequences(seed=5):
    """Three sequences: (ids [1, n], labels with the prompt masked) each."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for n in LENGTHS:
        ids = torch.randint(3, V, (1, n), generator=g)
        labels = ids.clone()
        labels[0, :PROMPT] = -100
        out.append((ids, labels))
    return out


def packed(seqs):
    ids = torch.cat([i for i, _ in seqs], dim=1)
    labels = torch.cat([lab for _, lab in seqs], dim=1)
    pos = torch.cat([torch.arange(i.shape[1]) for i, _ in seqs])[None]
    return ids, pos, labels


def nll_sum(logits, labels):
    """Summed negative log-probability of the labelled tokens of ONE sequence (fp32 at least)."""
    logits = logits[0, :-1]
    logits = logits.double() if logits.dtype == torch.float64 else logits.float()
    return F.cross_entropy(logits, labels[0, 1:].to(logits.device), ignore_index=-100, reduction="sum")


def per_sequence(model, seqs, dev):
    """Loss and gradients of the model run on each sequence alone, summed."""
    model.zero_grad()
    total = 0.0
    for ids, labels in seqs:
        loss = nll_sum(model(input_ids=ids.to(dev), attention_mask=torch.ones_like(ids).to(dev)).logits, labels)
        loss.backward()
        total = total + loss.detach()
    return total, {n: p.grad.detach().clone() for n, p in model.named_parameters()}


def packed_run(model, seqs, dev):
    """The same sum from ONE packed [1, T] row: the first token of a sequence is not a target of the sequence before it."""
    model.zero_grad()
    ids, pos, labels = packed(seqs)
    logits = model(input_ids=ids.to(dev), position_ids=pos.to(dev), attention_mask=torch.ones_like(ids).to(dev)).logits
    loss, at = 0.0, 0
    for i, lab in seqs:
        n = i.shape[1]
        loss = loss + nll_sum(logits[:, at:at + n], lab)
        at += n
    loss.backward()
    return loss.detach(), {n: p.grad.detach().clone() for n, p in model.named_parameters()}


def rel_err(got, want):
    return float((got.detach().double().cpu() - want).abs().max() / want.abs().max())


def counting(monkeypatch):
    calls = []
    real = fa.varlen_attention

    def counted(*a, **k):
        calls.append(1)
        return real(*a, **k)

    monkeypatch.setattr(fa, "varlen_attention", counted)
    return calls


@pytest.mark.parametrize("kind", ["qwen2", "llama"])
def test_packed_installed_model_is_as_close_to_fp64_as_the_stock_model_run_per_sequence(libprl, cuda_device, monkeypatch, kind):
    seqs = sequences()
    stock = tiny(kind)
    want_loss, want = per_sequence(fp64_copy(stock), seqs, "cpu")
    stock = stock.to(cuda_device)
    fused = install_fused_attention(copy.deepcopy(stock))
    assert fused._prl_fused_attention == {"previous": "sdpa", "layers": 2, "skipped": []}
    s_loss, s_grads = per_sequence(stock, seqs, cuda_device)
    calls = counting(monkeypatch)
    f_loss, f_grads = packed_run(fused, seqs, cuda_device)
    assert len(calls) == 2  # both layers took the kernels
    assert list(f_grads) == list(want)
    failed = []
    for name, got_f, got_s, w in [("loss", f_loss, s_loss, want_loss.reshape(1))] + [(n, f_grads[n], s_grads[n], want[n]) for n in want]:
        ef, es = rel_err(got_f.reshape(w.shape), w), rel_err(got_s.reshape(w.shape), w)
        print(f"[attention model {kind}] {name}: installed, packed {ef:.3e}  stock, per sequence {es:.3e}")
        if not ef <= MARGIN * es:
            failed.append(f"{name}: installed {ef:.3e} > {MARGIN:g} x stock {es:.3e}")
    assert not failed, "; ".join(failed)
    # for information: what the stock model makes of the packed row (every later sequence sees the earlier ones)
    p_loss, _ = packed_run(stock, seqs, cuda_device)
    print(f"[attention model {kind}] loss: stock sdpa on the packed row {rel_err(p_loss.reshape(1), want_loss.reshape(1)):.3e}")


def test_rl_step_with_head_body_and_attention(libprl, cuda_device, monkeypatch):
    from pipelinerl_amd.finetune.rl import RLConfig, rl_step
    from pipelinerl_amd.finetune.types import PipelineBatchEncoding
    from pipelinerl_amd.fused_head import install_fused_head, rl_step_fused_head

    seqs = sequences()
    ids, pos, labels = packed(seqs)
    labels = labels.clone()
    T = ids.shape[1]
    stock = tiny()
    wit = fp64_copy(stock)
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():  # fp64 log-probability of token t + 1, sequence by sequence; the last token of a sequence predicts nothing
        lps = []
        for i, _ in seqs:
            logits = wit(input_ids=i, attention_mask=torch.ones_like(i)).logits[0]
            lps.append(torch.cat([torch.log_softmax(logits[:-1], -1).gather(1, i[0, 1:, None])[:, 0], torch.zeros(1, dtype=torch.float64)]))
        lp = torch.cat(lps)[:-1]
    at = 0
    for n in LENGTHS:  # the first token of a packed sequence is never a target
        labels[0, at] = -100
        at += n
    old = (lp + 0.05 * torch.randn(T - 1, generator=g, dtype=torch.float64)).float()
    adv = torch.randn(T - 1, generator=g).float()
    mask = (labels[0, 1:] != -100).double()
    ratio = torch.exp(lp - old.double())
    want = -(torch.minimum(ratio * adv.double(), ratio.clamp(0.8, 1.2) * adv.double()) * mask / 8).sum()  # the PPO objective of RLConfig below

    def col(t):  # token-aligned [1, T]: column 0 predicts nothing
        return torch.cat([torch.zeros(1), t])[None].float()

    n_labels = float(mask.sum())
    batch = PipelineBatchEncoding(input_ids=ids, labels=labels, position_ids=pos, attention_mask=torch.ones_like(ids), old_logprobs=col(old),
                                  ref_logprobs=col(old), advantages=col(adv), rewards=torch.zeros(1, T), group_tokens=torch.full((1, T), n_labels),
                                  num_labels=torch.full((1, T), n_labels), overflow=torch.zeros(1, T), model_version=0,
                                  is_packed=True).to_device(cuda_device)
    cfg = RLConfig(policy_loss="ppo", epsilon_low=0.2, epsilon_high=0.2, kl_coef=0.0, final_kl_coef=0.0, batch_size=8, divide_advantage_by_std=False)
    alone = install_fused_attention(copy.deepcopy(stock).to(cuda_device))
    both = install_fused_attention(install_fused_body(install_fused_head(copy.deepcopy(stock).to(cuda_device))))
    calls = counting(monkeypatch)
    loss_a, stats_a = rl_step(alone, batch, 0, 10, cfg)
    loss_b, stats_b = rl_step_fused_head(both, batch, 0, 10, cfg)
    assert len(calls) == 4
    loss_b.backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in both.parameters())
    ea, eb = rel_err(loss_a.reshape(1), want.reshape(1)), rel_err(loss_b.reshape(1), want.reshape(1))
    print(f"[attention model] rl_step loss: head + body + attention {eb:.3e}, attention alone {ea:.3e} (fp64, per sequence {float(want):.9e})")
    assert eb <= MARGIN * ea, f"composed {eb:.3e} > {MARGIN:g} x attention alone {ea:.3e}"
