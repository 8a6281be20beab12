"""The fused gradient-norm / AdamW / Lion kernels (csrc/prl_optim.hip) and `pipelinerl_amd.finetune.optim` on the GPU.

Acceptance of a step is per entry, not by a max norm (tests/optim_checks.py): witness = the rule in fp64 on the CPU,
reference = the rule in fp32 on the CPU, an entry passes iff |k - wit| <= 4 r_ref scale with scale = the sum of the absolute
values of the entry's own terms and r_ref the reference's own worst relative error on those terms (floored at 2^-24).
The norm's bound is the fp64 summation error, N 2^-53 4 relative on the sum of squares (fp32 squares are exact in fp64)."""

import copy
import math
import types

import numpy as np
import pytest
import torch

from optim_checks import adamw_trajectory, check_entries, lion_trajectory, log_uniform_grads

pytestmark = pytest.mark.gpu

CHUNK = 16384
SIZES = [1, 7, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3] + [3 + 37 * k for k in range(60)]  # 69 + the unaligned view: two norm launches, three step launches


def build_params(device, rng, dtypes="mixed", grad_dtypes="mixed", steps=1):
    """The shape set: the sizes above + one view offset by ONE element (not 16-byte aligned), parameters ~N(0, 0.05), gradients of
    log-uniform scale.  Returns (params, grads[step][param] as numpy fp32 holding the values the device sees)."""
    params, grads = [], [[] for _ in range(steps)]
    for i, n in enumerate(SIZES + [1001]):
        unaligned = i == len(SIZES)
        pd = torch.float32 if dtypes == "f32" else torch.bfloat16 if dtypes == "bf16" else (torch.bfloat16 if i % 3 == 1 else torch.float32)
        gd = pd if grad_dtypes == "same" else (torch.float32 if i % 2 else pd)
        base = torch.from_numpy(rng.normal(0.0, 0.05, n + 1).astype(np.float32)).to(device=device, dtype=pd)
        p = torch.nn.Parameter(base[1:] if unaligned else base[:n].clone())
        assert (p.data_ptr() % 16 != 0) == unaligned
        p._grad_dtype, p._unaligned = gd, unaligned
        params.append(p)
        for s in range(steps):
            g = torch.from_numpy(log_uniform_grads(rng, n, 1)[0]).to(gd)
            grads[s].append(g.float().numpy())
    return params, grads


def set_grads(params, grads_step, device):
    for p, g in zip(params, grads_step):
        if g is None:
            p.grad = None
            continue
        t = torch.from_numpy(np.concatenate([[0.0], g]).astype(np.float32)).to(device=device, dtype=p._grad_dtype)
        if p._grad_dtype != p.dtype:
            p.grad_dtype = p._grad_dtype  # e.g. the fp32 d W of the fused head for a bf16 weight
        p.grad = t[1:] if p._unaligned else t[1:].clone()


def edges(n):
    idx = {0, n - 1}
    for c in range(CHUNK, n + 1, CHUNK):
        idx.update({c - 1, min(c, n - 1)})
    return sorted(idx)


def exact_sumsq(grads_step):
    return math.fsum(math.fsum((g.astype(np.float64).ravel() ** 2).tolist()) for g in grads_step if g is not None)


def test_grad_norm_bound_reproducibility_and_clip_coefficient(libprl, cuda_device):
    from pipelinerl_amd.finetune.optim import FusedAdamW

    rng = np.random.default_rng(101)
    params, grads = build_params(cuda_device, rng)
    assert len(params) > 64
    grads[0][5] = None  # a parameter without a gradient does not enter the norm
    set_grads(params, grads[0], cuda_device)
    opt = FusedAdamW(params, lr=1e-3)
    max_norm = 0.5
    norm = opt.compute_grad_norm(max_norm)
    assert norm.device.type == "cuda" and norm.dim() == 0
    rec1 = opt._record.clone()
    n_chunks = sum(-(-g.size // CHUNK) for g in grads[0] if g is not None)
    part1 = opt._workspace[: 8 * n_chunks].view(torch.float64).clone()
    want = exact_sumsq(grads[0])
    got = math.fsum(part1.cpu().tolist())
    N = sum(g.size for g in grads[0] if g is not None)
    rel = abs(got - want) / want
    print(f"[optim] norm: N = {N}, sum of squares rel. error {rel:.3e} (bound {N * 2.0 ** -53 * 4:.3e})")
    assert rel <= N * 2.0 ** -53 * 4
    # the record: fp32 of the root of the folded sum (the fold of n_chunks doubles adds at most n_chunks 2^-53), and torch's coefficient
    assert abs(float(rec1[0]) - math.sqrt(want)) <= 2.0 ** -23 * math.sqrt(want)
    coef = torch.clamp(torch.tensor(max_norm, dtype=torch.float32) / (rec1[0].cpu() + 1e-6), max=1.0)
    assert float(rec1[0]) > max_norm and rec1[1].cpu().view(torch.int32) == coef.view(torch.int32)
    # second run: bit-identical partials and record
    opt._workspace.zero_()
    opt.compute_grad_norm(max_norm)
    assert torch.equal(opt._record.view(torch.int32), rec1.view(torch.int32))
    assert torch.equal(opt._workspace[: 8 * n_chunks].view(torch.int64), part1.view(torch.int64))
    # below the threshold and "no clipping": coefficient exactly 1, the norm still reported
    for mn in (1e6, 0.0, None):
        opt.compute_grad_norm(mn)
        assert float(opt._record[1]) == 1.0 and opt._record[0].view(torch.int32) == rec1[0].view(torch.int32)
    # torch's own norm agrees to fp32 accuracy
    tn = torch.nn.utils.get_total_norm([p.grad.float() for p in params if p.grad is not None])
    assert abs(float(tn) - float(rec1[0])) <= 1e-5 * float(rec1[0])
    # a non-finite gradient propagates as it does in clip_grad_norm_
    params[0].grad[0] = float("nan")
    opt.compute_grad_norm(max_norm)
    assert torch.isnan(opt._record).all()


def _groups(params, wd=0.01):
    return [{"params": params[0::2], "weight_decay": wd}, {"params": params[1::2], "weight_decay": 0.0}]


def _wd_of(i, wd=0.01):
    return wd if i % 2 == 0 else 0.0


@pytest.mark.parametrize("dtypes", ["f32", "mixed"])
def test_adamw_step_per_entry(libprl, cuda_device, dtypes):
    from pipelinerl_amd.finetune.optim import FusedAdamW

    rng = np.random.default_rng(202)
    steps, lr = 3, 1e-3
    params, grads = build_params(cuda_device, rng, dtypes=dtypes, steps=steps)
    frozen = 4
    for s in range(steps):
        grads[s][frozen] = None  # never gets a gradient
    p0 = [p.detach().float().cpu().numpy().copy() for p in params]
    frozen_bits = params[frozen].detach().clone()
    opt = FusedAdamW(_groups(params), lr=lr, master_weights=True)
    coefs = []
    for s in range(steps):
        set_grads(params, grads[s], cuda_device)
        if s == 1:
            opt.step()  # plain step: coefficient 1
            coefs.append(1.0)
        else:
            opt.clip_and_step(0.05)
            coefs.append(float(opt._record[1]))
            assert coefs[-1] < 1.0
        opt.zero_grad()
    assert torch.equal(params[frozen].detach(), frozen_bits) and len(opt.state[params[frozen]]) == 0, "no gradient: parameter and state untouched"
    K, R, W, S = ([[], [], []] for _ in range(4))
    E = [[], [], []]
    bit_diff = 0
    for i, p in enumerate(params):
        if i == frozen:
            continue
        st = opt.state[p]
        assert float(st["step"]) == steps and st["exp_avg"].dtype == torch.float32
        g = [grads[s][i] for s in range(steps)]
        ref, _ = adamw_trajectory(p0[i], g, coefs, lr, _wd_of(i), dtype=torch.float32)
        wit, scales = adamw_trajectory(p0[i], g, coefs, lr, _wd_of(i), dtype=torch.float64)
        weights = st["master"] if "master" in st else p.detach()
        if p.dtype == torch.bfloat16:
            assert torch.equal(p.detach().view(torch.int16), st["master"].to(torch.bfloat16).view(torch.int16)), "bf16 parameter = RNE(master)"
        else:
            assert "master" not in st
        got = [weights.float().cpu().numpy().ravel(), st["exp_avg"].cpu().numpy().ravel(), st["exp_avg_sq"].cpu().numpy().ravel()]
        bit_diff += int((got[0].view(np.uint32) != ref[-1][0].view(np.uint32)).sum())
        e = edges(p.numel())
        for q in range(3):
            K[q].append(got[q]); R[q].append(ref[-1][q]); W[q].append(wit[-1][q]); S[q].append(scales[-1][q])
            E[q].append((got[q][e], ref[-1][q][e], wit[-1][q][e], scales[-1][q][e]))
    print(f"[optim] adamw {dtypes}: {bit_diff} weight entries differ in bits from torch's fp32 CPU AdamW (its sqrt is not the IEEE root)")
    for q, name in enumerate(("weights", "exp_avg", "exp_avg_sq")):
        r = check_entries(f"gpu adamw {dtypes} {name}", np.concatenate(K[q]), np.concatenate(R[q]), np.concatenate(W[q]), np.concatenate(S[q]))
        check_entries(f"gpu adamw {dtypes} {name} (first / last entry of every chunk and tensor)", *(np.concatenate([e[j] for e in E[q]]) for j in range(4)), r_ref=r)


def test_lion_step_per_entry(libprl, cuda_device):
    from pipelinerl_amd.finetune.optim import FusedLion

    rng = np.random.default_rng(303)
    steps, lr = 3, 1e-4
    params, grads = build_params(cuda_device, rng, dtypes="mixed", steps=steps)
    p0 = [p.detach().float().cpu().numpy().copy() for p in params]
    opt = FusedLion(_groups(params), lr=lr)
    coefs = []
    for s in range(steps):
        set_grads(params, grads[s], cuda_device)
        opt.clip_and_step(0.05 if s != 1 else None)
        coefs.append(float(opt._record[1]))
        opt.zero_grad()
    assert coefs[0] < 1.0 and coefs[1] == 1.0
    K, R, W, S, keep = ([[], []] for _ in range(5))
    for i, p in enumerate(params):
        st = opt.state[p]
        assert "exp_avg_sq" not in st
        g = [grads[s][i] for s in range(steps)]
        zeros = np.zeros_like(p0[i])
        ref, _ = lion_trajectory(p0[i], zeros, g, coefs, lr, _wd_of(i), dtype=np.float32)
        wit, scales = lion_trajectory(p0[i], zeros, g, coefs, lr, _wd_of(i), dtype=np.float64)
        decided = np.logical_and.reduce([w[2] for w in wit] + [r[2] for r in ref])
        weights = st["master"] if "master" in st else p.detach()
        got = [weights.float().cpu().numpy().ravel(), st["exp_avg"].cpu().numpy().ravel()]
        for q in range(2):
            K[q].append(got[q]); R[q].append(ref[-1][q]); W[q].append(wit[-1][q]); S[q].append(scales[-1][q])
            keep[q].append(decided if q == 0 else np.ones_like(decided))
    left_out = 1.0 - np.concatenate(keep[0]).mean()
    print(f"[optim] lion: {left_out:.4%} of the entries have a sign within rounding of zero and are left out of the weight comparison")
    assert left_out <= 0.001
    for q, name in enumerate(("weights", "exp_avg")):
        check_entries(f"gpu lion {name}", np.concatenate(K[q]), np.concatenate(R[q]), np.concatenate(W[q]), np.concatenate(S[q]), keep=np.concatenate(keep[q]))


def test_master_weights_keep_updates_that_bf16_rounds_away(libprl, cuda_device):
    from pipelinerl_amd.finetune.optim import FusedAdamW

    rng = np.random.default_rng(404)
    n, steps, lr = 50_000, 20, 1e-6
    p0 = torch.from_numpy(rng.normal(0.0, 0.05, n).astype(np.float32)).to(torch.bfloat16)
    sign = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    grads = [torch.from_numpy(g).to(torch.bfloat16) for g in log_uniform_grads(rng, n, steps, sign=sign)]
    # the stock path: torch.optim.AdamW on the bf16 parameter
    stock = torch.nn.Parameter(p0.clone())
    so = torch.optim.AdamW([stock], lr=lr, weight_decay=0.0, foreach=False)
    for g in grads:
        stock.grad = g.clone()
        so.step()
    unchanged = (stock.detach().view(torch.int16) == p0.view(torch.int16)).float().mean().item()
    print(f"[optim] stock bf16 AdamW, lr {lr}, {steps} steps: {unchanged:.2%} of the entries never moved")
    assert unchanged > 0.90
    p = torch.nn.Parameter(p0.clone().to(cuda_device))
    opt = FusedAdamW([p], lr=lr, weight_decay=0.0, master_weights=True)
    for g in grads:
        p.grad = g.to(cuda_device)
        opt.step()
    g32 = [g.float().numpy() for g in grads]
    ref, _ = adamw_trajectory(p0.float().numpy(), g32, [1.0] * steps, lr, 0.0, dtype=torch.float32)
    wit, scales = adamw_trajectory(p0.float().numpy(), g32, [1.0] * steps, lr, 0.0, dtype=torch.float64)
    st = opt.state[p]
    check_entries("gpu adamw master after 20 steps", st["master"].cpu().numpy(), ref[-1][0], wit[-1][0], scales[-1][0])
    assert torch.equal(p.detach().view(torch.int16), st["master"].to(torch.bfloat16).view(torch.int16))
    moved = (st["master"].cpu() != p0.float()).float().mean().item()
    assert moved > 0.99, "the master copy carries the updates the bf16 parameter cannot"
    drift = ((st["master"].cpu().double() - p0.double()) * torch.from_numpy(sign)).mean().item()
    assert drift < 0.0, "a constant gradient sign moves the master against it"


def test_clip_and_step_equals_clip_grad_norm_then_step(libprl, cuda_device):
    from pipelinerl_amd.finetune.optim import FusedAdamW

    for max_norm in (0.05, 1e6):  # the norm exceeds the threshold / it does not
        rng = np.random.default_rng(505)
        params, grads = build_params(cuda_device, rng, dtypes="f32", grad_dtypes="same")
        twins = [torch.nn.Parameter(p.detach().clone()) for p in params]
        for t, p in zip(twins, params):
            t._grad_dtype, t._unaligned = p._grad_dtype, False
        p0 = [p.detach().cpu().numpy().copy() for p in params]
        a, b = FusedAdamW(_groups(params), lr=1e-3), FusedAdamW(_groups(twins), lr=1e-3)
        set_grads(params, grads[0], cuda_device)
        set_grads(twins, grads[0], cuda_device)
        norm = a.clip_and_step(max_norm)
        tn = torch.nn.utils.clip_grad_norm_(twins, max_norm)
        b.step()
        assert abs(float(norm) - float(tn)) <= 1e-6 * float(tn)
        coef = float(a._record[1])
        assert (coef < 1.0) == (max_norm < 1.0)
        assert torch.equal(params[3].grad.cpu(), torch.from_numpy(grads[0][3])), "clip_and_step leaves the gradients as they were"
        K, K2, R, W, S = [], [], [], [], []
        for i, (p, t) in enumerate(zip(params, twins)):
            ref, _ = adamw_trajectory(p0[i], [grads[0][i]], [coef], 1e-3, _wd_of(i), dtype=torch.float32)
            wit, scales = adamw_trajectory(p0[i], [grads[0][i]], [coef], 1e-3, _wd_of(i), dtype=torch.float64)
            K.append(p.detach().cpu().numpy()); K2.append(t.detach().cpu().numpy()); R.append(ref[0][0]); W.append(wit[0][0]); S.append(scales[0][0])
        check_entries(f"clip_and_step({max_norm})", np.concatenate(K), np.concatenate(R), np.concatenate(W), np.concatenate(S))
        check_entries(f"clip_grad_norm_({max_norm}) + step", np.concatenate(K2), np.concatenate(R), np.concatenate(W), np.concatenate(S))


def test_rehomed_parameters_are_updated_in_place(libprl, cuda_device, monkeypatch):
    from pipelinerl_amd import weight_sync
    from pipelinerl_amd.finetune.optim import FusedAdamW

    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(64, 96), torch.nn.Linear(96, 32)).to(cuda_device).to(torch.bfloat16)
    tx = weight_sync.ColocatedSender(cuda_device, bucket_bytes=1 << 20)
    try:
        opt = FusedAdamW(model.parameters(), lr=1e-2)
        tx.rehome(model.named_parameters())
        before = [p.detach().clone() for p in model.parameters()]
        ptrs = [p.data_ptr() for p in model.parameters()]
        model(torch.randn(8, 64, device=cuda_device, dtype=torch.bfloat16)).float().pow(2).sum().backward()
        opt.clip_and_step(1.0)
        assert [p.data_ptr() for p in model.parameters()] == ptrs
        assert all(not torch.equal(a, p.detach()) for a, p in zip(before, model.parameters()))
        calls = []
        monkeypatch.setattr(weight_sync, "gather_into_bucket", lambda *a, **k: calls.append(a))
        tx.publish(model.named_parameters())
        assert not calls, "publish moves nothing: the step wrote the parameters where they live, inside the exported bucket"
        for p in model.parameters():
            home = [bk for bk in tx._buckets if bk.ptr <= p.data_ptr() < bk.ptr + bk.nbytes]
            assert len(home) == 1
            off = p.data_ptr() - home[0].ptr
            raw = home[0].tensor()[off: off + p.numel() * 2].clone().view(torch.bfloat16).view(p.shape)
            assert torch.equal(raw.view(torch.int16), p.detach().view(torch.int16))
            assert torch.equal(p.detach().view(torch.int16), opt.state[p]["master"].to(torch.bfloat16).view(torch.int16))
    finally:
        tx.close()


def test_fused_head_is_invalidated_by_clip_and_step(libprl, cuda_device):
    from pipelinerl_amd.finetune.optim import FusedAdamW, FusedLion
    from pipelinerl_amd.fused_head import FusedLmHead

    for cls in (FusedAdamW, FusedLion):
        w = torch.nn.Parameter(torch.randn(256, 64, device=cuda_device))
        head = FusedLmHead(w)
        opt = cls([w], lr=1e-3)
        head.attach_optimizer(opt)
        for call in (lambda: opt.clip_and_step(1.0), opt.step):
            head._key = "prepared"
            w.grad = torch.randn_like(w)
            call()
            assert head._key is None


def test_state_dict_round_trip_and_torch_checkpoint(libprl, cuda_device):
    from pipelinerl_amd.finetune.optim import FusedAdamW, FusedLion

    for cls in (FusedAdamW, FusedLion):
        rng = np.random.default_rng(606)
        params, grads = build_params(cuda_device, rng, dtypes="mixed", steps=3)
        opt = cls(_groups(params), lr=1e-3)
        for s in range(2):
            set_grads(params, grads[s], cuda_device)
            opt.clip_and_step(0.05)
        sd = copy.deepcopy(opt.state_dict())
        assert set(sd["state"][0]) == set(opt._state_keys) | {"step"} | ({"master"} if params[0].dtype == torch.bfloat16 else set())
        twins = [torch.nn.Parameter(p.detach().clone()) for p in params]
        for t, p in zip(twins, params):
            t._grad_dtype, t._unaligned = p._grad_dtype, False
        opt2 = cls(_groups(twins), lr=123.0)
        opt2.load_state_dict(sd)
        assert opt2.param_groups[0]["lr"] == 1e-3
        set_grads(params, grads[2], cuda_device)
        set_grads(twins, grads[2], cuda_device)
        opt.clip_and_step(0.05)
        opt2.clip_and_step(0.05)
        for p, t in zip(params, twins):
            assert torch.equal(p.detach().view(torch.uint8), t.detach().view(torch.uint8))
            for k in opt.state[p]:
                a, b = opt.state[p][k], opt2.state[t][k]
                assert a.dtype == b.dtype and torch.equal(a.cpu(), b.cpu()), k
    # a torch.optim.AdamW checkpoint of fp32 parameters loads (same keys) and continues from its step count
    w = torch.nn.Parameter(torch.randn(1000, device=cuda_device))
    w2 = torch.nn.Parameter(w.detach().clone())
    ta = torch.optim.AdamW([w], lr=1e-3, foreach=False)
    g = torch.randn(2, 1000, device=cuda_device)
    w.grad = g[0].clone()
    ta.step()
    w2.data.copy_(w.detach())
    fa = FusedAdamW([w2], lr=1e-3)
    fa.load_state_dict(copy.deepcopy(ta.state_dict()))
    w.grad, w2.grad = g[1].clone(), g[1].clone()
    ta.step()
    fa.step()
    assert float(fa.state[w2]["step"]) == 2.0
    assert torch.allclose(w2.detach(), w.detach(), rtol=0, atol=1e-6) and torch.allclose(fa.state[w2]["exp_avg"], ta.state[w]["exp_avg"], rtol=1e-6, atol=0)


class TinyLM(torch.nn.Module):  # the tiny fp32 model of tests/test_gpu_pipeline.py
    def __init__(self, vocab=64, dim=16):
        super().__init__()
        self.emb = torch.nn.Embedding(vocab, dim)
        self.head = torch.nn.Linear(dim, vocab)

    def forward(self, input_ids=None, **kw):
        return types.SimpleNamespace(logits=self.head(self.emb(input_ids)).float())


class TinyHFLM(torch.nn.Module):
    """Hugging Face layout for `install_fused_head`: `.model` returns the last hidden states (bf16), `.lm_head` is a bias-free Linear."""

    class Body(torch.nn.Module):
        def __init__(self, vocab, dim):
            super().__init__()
            self.emb = torch.nn.Embedding(vocab, dim)

        def forward(self, input_ids=None, **kw):
            return (torch.tanh(self.emb(input_ids)).to(torch.bfloat16),)

    def __init__(self, vocab=128, dim=64):
        super().__init__()
        self.model = TinyHFLM.Body(vocab, dim)
        self.lm_head = torch.nn.Linear(dim, vocab, bias=False)


@pytest.mark.parametrize("learner", ["plain", "native", "streamed"])
def test_learner_step_with_fused_adamw_matches_torch_adamw(libprl, cuda_device, tmp_path, learner):
    from pipelinerl_amd import streams
    from pipelinerl_amd.finetune.optim import FusedAdamW
    from pipelinerl_amd.finetune.rl import RLConfig
    from pipelinerl_amd.finetune_loop import TRAINER_TOPIC, LearnerStep, NativeLearnerStep, StreamedLearnerStep
    from pipelinerl_amd.fused_head import install_fused_head
    from pipelinerl_amd.hotpath import HotPathStep, dense_micro_batches
    from pipelinerl_amd.synthetic import make_ragged

    V, lr, thr, wd = 128, 1e-3, 0.05, 0.01
    rag_h, _ = make_ragged(4, attempts=4, seq_length=40, vocab=V, seed=3, prompt_min=3, prompt_max=8, with_ref=True)
    rag = rag_h.to(cuda_device)
    mbs = dense_micro_batches(rag_h, 100)
    rl = RLConfig(policy_loss="ppo", epsilon_low=0.2, epsilon_high=0.2, kl_coef=0.05, final_kl_coef=0.05, divide_advantage_by_std=True,
                  clamp_log_ratio_ref_new_value=5)
    cfg = rl.model_copy()
    cfg.batch_size = 16
    batches = HotPathStep(cfg, 2, 0, 10).preprocess(rag, mbs)
    torch.manual_seed(0)
    if learner == "streamed":  # (a deep copy of an installed model would keep the forward bound to the original)
        raw = [TinyHFLM(V).to(cuda_device)]
        raw.append(copy.deepcopy(raw[0]))
        models = [install_fused_head(m) for m in raw]
    else:
        models = [TinyLM(V).to(cuda_device)]
        models.append(copy.deepcopy(models[0]))
    p0 = [p.detach().cpu().numpy().copy() for p in models[0].parameters()]
    opts = [FusedAdamW(models[0].parameters(), lr=lr, weight_decay=wd), torch.optim.AdamW(models[1].parameters(), lr=lr, weight_decay=wd, foreach=False)]
    norms, seen = [[], []], []
    for k, (model, opt) in enumerate(zip(models, opts)):
        streams.reset_streams_backend()
        streams.set_streams_backend("files")
        if k == 0:  # the gradients the fused step consumed, for the witness
            zero = opt.zero_grad
            opt.zero_grad = lambda *a, _z=zero, _m=model, **kw: seen.append([p.grad.detach().cpu().numpy().copy() for p in _m.parameters()]) or _z(*a, **kw)
        (tmp_path / f"run{k}").mkdir(exist_ok=True)
        if learner == "native":
            step = NativeLearnerStep(model, opt, rl, eos_token_id=2, samples_per_step=16, max_train_steps=10, gradient_clipping_threshold=thr)
        else:
            step = (StreamedLearnerStep if learner == "streamed" else LearnerStep)(model, opt, rl, train_batch_size=1, gradient_accumulation_passes=16, max_train_steps=10, send_weight_updates=False,
                gradient_clipping_threshold=thr, trainer_stream=streams.SingleStreamSpec(exp_path=tmp_path / f"run{k}", topic=TRAINER_TOPIC))
        for _ in range(2):
            if learner == "native":
                assert step.step(rag, mbs)["did_optimizer_step"]
            else:
                for i, b in enumerate(batches):
                    res = step.step(b)
                    assert res["did_optimizer_step"] == (i == len(batches) - 1)
            norms[k].append(step.metrics.grad_norm)
        assert step.metrics.completed_steps == 2
    streams.reset_streams_backend()
    assert len(seen) == 2
    for s in range(2):
        exact = math.sqrt(exact_sumsq(seen[s]))
        assert abs(norms[0][s] - exact) <= 1e-6 * exact, "the fused norm against the fp64 sum of the same gradients"
    assert abs(norms[0][0] - norms[1][0]) <= 1e-6 * norms[1][0], "same grad_norm as clip_grad_norm_ (step 1: identical gradients)"
    coefs = [float(np.float32(thr) / (np.float32(n) + np.float32(1e-6))) if n > thr else 1.0 for n in norms[0]]
    K, R, W, S, gap = [], [], [], [], 0.0
    for i, (pa, pb) in enumerate(zip(models[0].parameters(), models[1].parameters())):
        g = [seen[0][i].ravel(), seen[1][i].ravel()]
        ref, _ = adamw_trajectory(p0[i].ravel(), g, coefs, lr, wd, dtype=torch.float32)
        wit, scales = adamw_trajectory(p0[i].ravel(), g, coefs, lr, wd, dtype=torch.float64)
        K.append(pa.detach().cpu().numpy().ravel()); R.append(ref[-1][0]); W.append(wit[-1][0]); S.append(scales[-1][0])
        gap = max(gap, float((pa.detach() - pb.detach()).abs().max()))
    check_entries(f"LearnerStep ({learner}) + FusedAdamW, 2 steps", np.concatenate(K), np.concatenate(R), np.concatenate(W), np.concatenate(S))
    # the model trained by torch.optim.AdamW through its own learner step: its step-2 gradients come from parameters that already differ
    # by rounding, so it is compared on its own.  One AdamW step moves an entry by at most lr (1 - b1) / sqrt(1 - b2) = 3.2 lr (+ the
    # decay); two models that took the same two steps up to rounding stay far inside one such step of each other.
    print(f"[optim] LearnerStep ({learner}): largest distance between the FusedAdamW and the torch.optim.AdamW model after 2 steps = {gap / lr:.3e} lr")
    assert gap <= 3.2 * lr
