"""`install_fused_body` on a tiny Qwen2ForCausalLM on the GPU: loss and every parameter gradient of the installed model and of
the stock model against an fp64 copy of the model on the CPU.  Per tensor, with err = max |got - want| / max |want|, the
installed model may be at most 4 x as far from fp64 as the stock model is (the project's standing margin).  With
`install_fused_head` as well, `rl_step_fused_head` runs and its loss meets the same criterion against the fused-head-only model."""

import copy

import pytest
import torch
import torch.nn.functional as F

from pipelinerl_amd.fused_body import RMSNORM_CLASSES, install_fused_body

transformers = pytest.importorskip("transformers")
pytestmark = pytest.mark.gpu

V, LENGTHS, PROMPT = 512, (17, 23, 24), 4
MARGIN = 4.0


def tiny_qwen2(dtype):
    cfg = transformers.Qwen2Config(vocab_size=V, hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=4,
                                   num_key_value_heads=2, max_position_embeddings=256, tie_word_embeddings=False, attn_implementation="eager")
    torch.manual_seed(0)
    return transformers.Qwen2ForCausalLM(cfg).to(dtype)


def fp64_copy(model):
    """The model in fp64 on the CPU.  transformers' RMSNorm computes in fp32 whatever it is given: in the witness its formula
    runs in fp64 like everything else."""
    wit = copy.deepcopy(model).double().cpu()
    for m in wit.modules():
        if type(m).__name__ in RMSNORM_CLASSES:
            m.forward = lambda h, m=m: m.weight * (h * torch.rsqrt(h.pow(2).mean(-1, keepdim=True) + m.variance_epsilon))
    return wit


def packed_inputs(seed=5):
    """Three sequences packed into one row: ids, positions restarting per sequence, labels with every prompt masked."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(3, V, (1, sum(LENGTHS)), generator=g)
    pos = torch.cat([torch.arange(n) for n in LENGTHS])[None]
    labels = ids.clone()
    start = 0
    for n in LENGTHS:
        labels[0, start:start + PROMPT] = -100
        start += n
    return ids, pos, labels


def token_loss(model, ids, pos, labels, dev):
    """Mean negative log-probability of the labelled tokens, from the model's logits in the model's arithmetic (fp32 at least)."""
    logits = model(input_ids=ids.to(dev), position_ids=pos.to(dev), attention_mask=torch.ones_like(ids).to(dev)).logits[0, :-1]
    logits = logits.double() if logits.dtype == torch.float64 else logits.float()
    target = labels[0, 1:].to(dev)
    return F.cross_entropy(logits, target, ignore_index=-100)


def rel_err(got, want):
    return float((got.detach().double().cpu() - want).abs().max() / want.abs().max())


def loss_and_grads(model, ids, pos, labels, dev):
    model.zero_grad()
    loss = token_loss(model, ids, pos, labels, dev)
    loss.backward()
    return loss.detach(), {n: p.grad.detach() for n, p in model.named_parameters()}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_installed_model_is_as_close_to_fp64_as_the_stock_model(libprl, cuda_device, dtype):
    ids, pos, labels = packed_inputs()
    stock = tiny_qwen2(dtype)
    want_loss, want = loss_and_grads(fp64_copy(stock), ids, pos, labels, "cpu")
    stock = stock.to(cuda_device)
    fused = install_fused_body(copy.deepcopy(stock))
    assert fused._prl_fused_body["rmsnorm"] == 5 and fused._prl_fused_body["swiglu"] == 2
    s_loss, s_grads = loss_and_grads(stock, ids, pos, labels, cuda_device)
    f_loss, f_grads = loss_and_grads(fused, ids, pos, labels, cuda_device)
    assert list(f_grads) == list(want)
    failed = []
    for name, got_f, got_s, w in [("loss", f_loss, s_loss, want_loss.reshape(1))] + [(n, f_grads[n], s_grads[n], want[n]) for n in want]:
        ef, es = rel_err(got_f.reshape(w.shape), w), rel_err(got_s.reshape(w.shape), w)
        print(f"[body model {dtype}] {name}: installed {ef:.3e} stock {es:.3e}")
        if not ef <= MARGIN * es:
            failed.append(f"{name}: installed {ef:.3e} > {MARGIN:g} x stock {es:.3e}")
    assert not failed, "; ".join(failed)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_rl_step_fused_head_with_the_fused_body(libprl, cuda_device, dtype):
    from pipelinerl_amd.finetune.rl import RLConfig
    from pipelinerl_amd.finetune.types import PipelineBatchEncoding
    from pipelinerl_amd.fused_head import install_fused_head, rl_step_fused_head

    ids, pos, labels = packed_inputs()
    T = ids.shape[1]
    stock = tiny_qwen2(dtype)
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():
        logits = fp64_copy(stock)(input_ids=ids, position_ids=pos, attention_mask=torch.ones_like(ids)).logits[0]
    lp = torch.log_softmax(logits[:-1], -1).gather(1, ids[0, 1:, None])[:, 0]  # fp64 log-probability of token t + 1
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
    head_only = install_fused_head(copy.deepcopy(stock).to(cuda_device))
    both = install_fused_body(install_fused_head(copy.deepcopy(stock).to(cuda_device)))
    loss_a, stats_a = rl_step_fused_head(head_only, batch, 0, 10, cfg)
    loss_b, stats_b = rl_step_fused_head(both, batch, 0, 10, cfg)
    loss_b.backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in both.parameters())
    assert list(stats_a) == list(stats_b)
    ea, eb = rel_err(loss_a.reshape(1), want.reshape(1)), rel_err(loss_b.reshape(1), want.reshape(1))
    print(f"[body model {dtype}] rl_step_fused_head loss: head + body {eb:.3e}, head only {ea:.3e} (fp64 {float(want):.9e})")
    assert eb <= MARGIN * ea, f"head + body {eb:.3e} > {MARGIN:g} x head only {ea:.3e}"
