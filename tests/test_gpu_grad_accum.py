"""fp32 gradient accumulation on the GPU: `grad_accumulate_kernel` (csrc/prl_optim.hip) through `prl_optim_grad_accumulate`, the
optimizer methods built on it (`accumulate_grads`, `reduce_accumulated`, norm / step reading the accumulators) and the three learner
steps driving them.

Everything here is an equality of bits: one fold is one IEEE fp32 add per element (a bf16 gradient widens exactly), every element is
owned by one lane, so the accumulator after k folds IS the sequential fp32 sum `((g0 + g1) + g2) + ...` that torch forms on the CPU,
and an optimizer that reads it takes the step of one that was handed that sum as an fp32 `p.grad` (a path tests/test_gpu_optim.py
already holds to the reference)."""

import copy
import math
import multiprocessing as mp
import os
import types

import numpy as np
import pytest
import torch

from optim_checks import log_uniform_grads

pytestmark = pytest.mark.gpu

CHUNK = 16384
SIZES = [1, 7, 8, 9, 63, 64, 65, 2047, 2048, 2049, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3] + [3 + 37 * k for k in range(60)]
GUARD = 16  # elements behind every accumulator that no fold may touch


def bits(t: torch.Tensor) -> torch.Tensor:
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int16)


def seq_sum(grads) -> torch.Tensor:
    """The sequential fp32 sum of CPU tensors (fp32 or bf16), in order."""
    acc = grads[0].float().clone()
    for g in grads[1:]:
        acc = acc + g.float()
    return acc


# ---- 1. the kernel -------------------------------------------------------------------------------------------------------------------
def test_kernel_is_the_sequential_fp32_sum_bit_for_bit(libprl, cuda_device):
    from pipelinerl_amd import _lib

    rng = np.random.default_rng(11)
    folds = 8
    # (numel, bf16 gradient?, gradient view off 16-byte alignment?, accumulator view off alignment?)
    cases = [(n, i % 2 == 0, False, False) for i, n in enumerate(SIZES)]
    cases += [(1001, True, True, False), (1003, False, True, False), (2051, True, False, True), (CHUNK + 5, False, True, True)]
    assert len(cases) > 64, "more than one launch per call"
    host, dev, accs = [], [], []
    for n, is_bf16, g_off, a_off in cases:
        dt = torch.bfloat16 if is_bf16 else torch.float32
        hs = [torch.from_numpy(g).to(dt) for g in log_uniform_grads(rng, n, folds)]
        host.append(hs)
        ds = []
        for h in hs:
            base = torch.zeros(n + 1, dtype=dt, device=cuda_device)
            view = base[1:] if g_off else base[:n]
            view.copy_(h)
            assert (view.data_ptr() % 16 != 0) == g_off
            ds.append(view)
        dev.append(ds)
        base = torch.full((n + 1 + GUARD,), float("nan"), dtype=torch.float32, device=cuda_device)
        base[-GUARD:] = 12345.0
        if a_off:
            base[0] = 12345.0
        acc = base[1:n + 1] if a_off else base[:n]
        assert (acc.data_ptr() % 16 != 0) == a_off
        accs.append((base, acc, a_off))
    want = [seq_sum(hs) for hs in host]
    stream = _lib.current_stream_ptr(cuda_device)
    runs = []
    for _ in range(2):
        for base, acc, _a in accs:
            acc.fill_(float("nan"))  # the overwriting fold must not read it
        for k in range(folds):
            table = (_lib.PrlAccumSegment * (len(cases) + 2))()
            for seg, (n, is_bf16, _g, _a), ds, (_b, acc, _o) in zip(table, cases, dev, accs):
                seg.grad, seg.acc, seg.numel = ds[k].data_ptr(), acc.data_ptr(), n
                seg.grad_dtype = _lib.PRL_DTYPE_BF16 if is_bf16 else _lib.PRL_DTYPE_F32
            table[len(cases)].numel = 100  # no gradient: skipped
            table[len(cases) + 1].grad, table[len(cases) + 1].acc = ds[k].data_ptr(), accs[0][1].data_ptr()  # numel 0: skipped
            _lib.check(libprl.prl_optim_grad_accumulate(table, len(table), int(k == 0), stream))
        torch.cuda.synchronize(cuda_device)
        runs.append([acc.cpu().clone() for _b, acc, _o in accs])
        for base, acc, a_off in accs:
            assert torch.all(base[-GUARD:] == 12345.0) and (not a_off or float(base[0]) == 12345.0), "a fold wrote outside its accumulator"
    for (n, is_bf16, g_off, a_off), w, r0, r1 in zip(cases, want, runs[0], runs[1]):
        assert not torch.isnan(r0).any()
        bad = (bits(r0) != bits(w)).nonzero().flatten()
        assert bad.numel() == 0, f"numel {n} bf16 {is_bf16} unaligned {g_off, a_off}: {bad.numel()} entries differ from the sequential fp32 sum, first at {int(bad[0])}"
        assert torch.equal(bits(r0), bits(r1)), "two runs, two results"


# ---- 2. the case bf16 loses ----------------------------------------------------------------------------------------------------------
def test_512_equal_gradients_sum_to_512_where_a_bf16_running_sum_stops_at_256(libprl, cuda_device):
    from pipelinerl_amd.finetune.optim import FusedAdamW

    n, passes = 3 * CHUNK + 17, 512
    p = torch.nn.Parameter(torch.zeros(n, dtype=torch.bfloat16, device=cuda_device))
    opt = FusedAdamW([p], lr=1e-3, grad_accum_dtype=torch.float32)
    g = torch.ones(n, dtype=torch.bfloat16, device=cuda_device)
    for _ in range(passes):
        p.grad = g.clone()  # what a backward leaves when p.grad was None
        opt.accumulate_grads()
        assert p.grad is None
    acc = opt._acc[p]
    assert acc.dtype == torch.float32 and acc.data_ptr() % 64 == 0
    assert torch.all(acc == 512.0), "every accumulator entry is exactly 512"
    # the way autograd sums them: p.grad += g in the parameter's dtype.  256 + 1 ties to even in an 8-bit significand.
    # (This assertion is about torch, not about this project: it documents why the accumulator exists.)
    p.grad = g.clone()
    for _ in range(passes - 1):
        p.grad += g
    assert torch.all(p.grad == 256.0)


# ---- 3. the optimizer ----------------------------------------------------------------------------------------------------------------
def build(device, rng, steps, micro):
    """A mixed list in the manner of `build_params` (tests/test_gpu_optim.py): bf16 parameters with bf16 gradients (folded), bf16
    parameters with fp32 gradients and fp32 parameters (both bypass the accumulator), one view off 16-byte alignment.
    Returns (params, grads[step][micro][param] as CPU tensors in the gradient's dtype, or None)."""
    params = []
    for i, n in enumerate(SIZES + [1001]):
        unaligned = i == len(SIZES)
        pd = torch.bfloat16 if (i % 3 != 0 or unaligned) else torch.float32
        gd = torch.float32 if (pd == torch.float32 or i % 5 == 1) else torch.bfloat16
        base = torch.from_numpy(rng.normal(0.0, 0.05, n + 1).astype(np.float32)).to(device=device, dtype=pd)
        p = torch.nn.Parameter(base[1:] if unaligned else base[:n].clone())
        assert (p.data_ptr() % 16 != 0) == unaligned
        p._gd, p._unaligned = gd, unaligned
        if gd != pd:
            p.grad_dtype = gd
        params.append(p)
    frozen, late = 4, 7  # never a gradient / a gradient from the fourth micro-batch on
    assert params[late].dtype == torch.bfloat16 and params[late]._gd == torch.bfloat16
    grads = [[[None if (i == frozen or (i == late and k < 3)) else torch.from_numpy(log_uniform_grads(rng, p.numel(), 1)[0]).to(p._gd)
               for i, p in enumerate(params)] for k in range(micro)] for _ in range(steps)]
    return params, grads, frozen


def give(p, g, device):
    """What a backward does: move the gradient in when there is none, add to it in its dtype otherwise."""
    if g is None:
        return
    if p.grad is None:
        t = torch.zeros(g.numel() + 1, dtype=g.dtype, device=device)
        view = t[1:] if p._unaligned else t[1:].clone()
        view.copy_(g)
        p.grad = view
    else:
        p.grad += g.to(device)


def twins_of(params):
    out = []
    for p in params:
        t = torch.nn.Parameter(p.detach().clone())
        t._gd, t._unaligned = torch.float32, False
        if t.dtype != torch.float32:
            t.grad_dtype = torch.float32
        out.append(t)
    return out


def groups(params):
    return [{"params": params[0::2], "weight_decay": 0.01}, {"params": params[1::2], "weight_decay": 0.0}]


@pytest.mark.parametrize("name", ["adamw", "lion"])
def test_accumulating_optimizer_equals_one_handed_the_fp32_sums(libprl, cuda_device, name):
    from pipelinerl_amd.finetune.optim import FusedAdamW, FusedLion

    cls = FusedAdamW if name == "adamw" else FusedLion
    rng = np.random.default_rng(21)
    steps, micro = 2, 16
    params, grads, frozen = build(cuda_device, rng, steps, micro)
    twins = twins_of(params)
    a = cls(groups(params), lr=1e-3, grad_accum_dtype=torch.float32)
    b = cls(groups(twins), lr=1e-3)
    folded = [p for p in params if p._gd != torch.float32]
    assert len(folded) > 20 and len(folded) < len(params) - 20
    for s in range(steps):
        for k in range(micro):
            for p, g in zip(params, grads[s][k]):
                give(p, g, cuda_device)
            a.accumulate_grads()
            assert all(p.grad is None for p in folded), "a folded gradient is cleared"
        assert a._acc_flat is not None and all(a._acc[p].data_ptr() % 64 == 0 for p in folded)
        assert set(a._acc) == set(folded), "fp32 gradients are not folded"
        for i, (p, t) in enumerate(zip(params, twins)):
            gs = [grads[s][k][i] for k in range(micro) if grads[s][k][i] is not None]
            t.grad = seq_sum(gs).to(cuda_device) if gs else None
            if p._gd == torch.float32 and gs:
                assert torch.equal(bits(p.grad), bits(t.grad)), "an fp32 gradient is left to autograd's own fp32 sum"
            elif gs:
                assert torch.equal(bits(a._grad_of(p)), bits(t.grad)), f"accumulator {i} is not the sequential fp32 sum"
        na, nb = a.clip_and_step(0.05), b.clip_and_step(0.05)
        assert float(a._record[1]) < 1.0 and torch.equal(bits(na), bits(nb)) and torch.equal(bits(a._record), bits(b._record))
        a.zero_grad()
        b.zero_grad()
        for i, (p, t) in enumerate(zip(params, twins)):
            assert torch.equal(bits(p), bits(t)), f"step {s + 1}: parameter {i}"
            sa, sb = a.state[p], b.state[t]
            assert set(sa) == set(sb) and (i != frozen or not sa)
            for key in sa:
                assert sa[key].dtype == sb[key].dtype and torch.equal(bits(sa[key].float()), bits(sb[key].float())), f"step {s + 1}: {key} of parameter {i}"
            if p.dtype == torch.bfloat16 and i != frozen:
                assert "master" in sa and ("exp_avg_sq" in sa) == (name == "adamw")


@pytest.mark.parametrize("name", ["adamw", "lion"])
def test_unfolded_gradient_zero_grad_and_state_dict(libprl, cuda_device, name):
    from pipelinerl_amd.finetune.optim import FusedAdamW, FusedLion

    cls = FusedAdamW if name == "adamw" else FusedLion
    rng = np.random.default_rng(31)
    n = CHUNK + 9
    w = torch.from_numpy(rng.normal(0, 0.05, n).astype(np.float32))
    g = [torch.from_numpy(x).to(torch.bfloat16) for x in log_uniform_grads(rng, n, 6)]
    p = torch.nn.Parameter(w.to(device=cuda_device, dtype=torch.bfloat16))
    q = torch.nn.Parameter(w.to(device=cuda_device))  # fp32: bypasses
    opt = cls([p, q], lr=1e-3, grad_accum_dtype=torch.float32)
    # an unfolded micro-batch is an error, not a dropped one
    p.grad = g[0].to(cuda_device)
    opt.accumulate_grads()
    p.grad = g[1].to(cuda_device)
    before = p.detach().clone()
    for call in (opt.step, lambda: opt.clip_and_step(1.0), lambda: opt.compute_grad_norm(1.0)):
        with pytest.raises(RuntimeError, match="accumulate_grads"):
            call()
    assert torch.equal(bits(p), bits(before)) and not opt.state[p]
    opt.accumulate_grads()
    assert torch.equal(bits(opt._grad_of(p)), bits(g[0].float() + g[1].float()))
    # zero_grad empties the accumulator without touching it: the next fold overwrites, and until then there is no gradient
    opt._acc[p].fill_(float("nan"))
    opt.zero_grad()
    assert opt._grad_of(p) is None
    opt.step()
    assert torch.equal(bits(p), bits(before)) and not opt.state[p], "never folded since zero_grad: skipped like a None gradient"
    p.grad = g[2].to(cuda_device)
    opt.accumulate_grads(set_to_none=False)
    assert p.grad is not None and torch.all(p.grad == 0), "set_to_none=False zeroes in place"
    assert torch.equal(bits(opt._grad_of(p)), bits(g[2].float()))
    p.grad += g[3].to(cuda_device)  # the next backward adds to the zeroed gradient
    with pytest.raises(RuntimeError, match="accumulate_grads"):
        opt.step()
    opt.accumulate_grads(set_to_none=False)
    assert torch.equal(bits(opt._grad_of(p)), bits(g[2].float() + g[3].float()))
    q.grad = g[2].float().to(cuda_device)
    opt.clip_and_step(0.05)  # a zeroed, folded p.grad is not "unfolded"
    assert opt._grad_of(p) is p.grad, "after a step the accumulator is empty again"
    opt.zero_grad()
    # the accumulators are transient: not in the state dict, which loads into an optimizer with or without the option
    sd = copy.deepcopy(opt.state_dict())
    assert set(sd["state"][0]) == set(opt._state_keys) | {"step", "master"} and set(sd["state"][1]) == set(opt._state_keys) | {"step"}
    n_acc = opt._acc_flat.numel()
    assert all(not (isinstance(v, torch.Tensor) and v.numel() == n_acc) for st in sd["state"].values() for v in st.values())
    p2, q2 = torch.nn.Parameter(p.detach().clone()), torch.nn.Parameter(q.detach().clone())
    p3, q3 = torch.nn.Parameter(p.detach().clone()), torch.nn.Parameter(q.detach().clone())
    p3.grad_dtype = torch.float32
    opt2 = cls([p2, q2], lr=123.0, grad_accum_dtype=torch.float32)
    opt3 = cls([p3, q3], lr=123.0)
    opt2.load_state_dict(sd)
    opt3.load_state_dict(copy.deepcopy(sd))
    for o, (pp, qq) in ((opt, (p, q)), (opt2, (p2, q2))):
        for k in (4, 5):
            pp.grad = g[k].to(cuda_device)
            o.accumulate_grads()
        qq.grad = g[4].float().to(cuda_device)
        o.clip_and_step(0.05)
    p3.grad, q3.grad = (g[4].float() + g[5].float()).to(cuda_device), g[4].float().to(cuda_device)
    opt3.clip_and_step(0.05)
    for pp, qq, o in ((p2, q2, opt2), (p3, q3, opt3)):
        assert torch.equal(bits(pp), bits(p)) and torch.equal(bits(qq), bits(q))
        for key in opt.state[p]:
            assert torch.equal(bits(o.state[pp][key].float()), bits(opt.state[p][key].float())), key


# ---- 4. the learner steps --------------------------------------------------------------------------------------------------------------
class TinyLM(torch.nn.Module):  # the tiny model of tests/test_gpu_optim.py
    def __init__(self, vocab=64, dim=16):
        super().__init__()
        self.emb = torch.nn.Embedding(vocab, dim)
        self.head = torch.nn.Linear(dim, vocab)

    def forward(self, input_ids=None, **kw):
        return types.SimpleNamespace(logits=self.head(self.emb(input_ids)).float())


class TinyHFLM(torch.nn.Module):
    """Hugging Face layout for `install_fused_head`: `.model` returns the last hidden states (bf16), `.lm_head` is a bias-free fp32 Linear."""

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
def test_learner_steps_fold_every_micro_batch(libprl, cuda_device, tmp_path, learner):
    """A bf16 body under each learner step with `FusedAdamW(grad_accum_dtype=torch.float32)`: what the step consumes is the sequential
    fp32 sum of the gradients each backward left, `p.grad` is None after each fold, and the reported norm is that of those sums.
    The gradients are captured where every step reads them: `compute_grad_norm`, which `clip_and_step` calls and which
    `StreamedLearnerStep` calls on its own before `step(clipped=True)`."""
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
    if learner == "streamed":
        raw = TinyHFLM(V).to(cuda_device)
        raw.model.to(torch.bfloat16)  # the body in bf16, the head stays fp32 (its gradient bypasses the accumulator)
        model = install_fused_head(raw)
    else:
        model = TinyLM(V).to(cuda_device).to(torch.bfloat16)
    params = list(model.parameters())
    body = [p for p in params if p.dtype == torch.bfloat16]
    assert body and (learner != "streamed" or len(body) < len(params))
    opt = FusedAdamW(params, lr=lr, weight_decay=wd, grad_accum_dtype=torch.float32)  # without the feature: TypeError here
    seen, consumed = [], []
    fold, norm = opt.accumulate_grads, opt.compute_grad_norm

    def recording_fold(*a, **kw):
        seen.append([None if p.grad is None else p.grad.detach().cpu().clone() for p in params])
        fold(*a, **kw)
        assert all(p.grad is None for p in body), "p.grad is None after each fold"

    def recording_norm(*a, **kw):
        consumed.append(([None if opt._grad_of(p) is None else opt._grad_of(p).detach().cpu().clone() for p in params], len(seen)))
        return norm(*a, **kw)

    opt.accumulate_grads, opt.compute_grad_norm = recording_fold, recording_norm
    streams.reset_streams_backend()
    streams.set_streams_backend("files")
    if learner == "native":
        step = NativeLearnerStep(model, opt, rl, eos_token_id=2, samples_per_step=16, max_train_steps=10, gradient_clipping_threshold=thr)
    else:
        step = (StreamedLearnerStep if learner == "streamed" else LearnerStep)(model, opt, rl, train_batch_size=1, gradient_accumulation_passes=16,
            max_train_steps=10, send_weight_updates=False, gradient_clipping_threshold=thr,
            trainer_stream=streams.SingleStreamSpec(exp_path=tmp_path, topic=TRAINER_TOPIC))
    assert step.fp32_accumulation
    norms = []
    for _ in range(2):
        if learner == "native":
            assert step.step(rag, mbs)["did_optimizer_step"]
        else:
            for i, b in enumerate(batches):
                assert step.step(b)["did_optimizer_step"] == (i == len(batches) - 1)
        norms.append(step.metrics.grad_norm)
    streams.reset_streams_backend()
    assert step.metrics.completed_steps == 2 and len(consumed) == 2 and len(seen) == 2 * len(batches) and len(batches) > 4
    first = 0
    for s, (accs, upto) in enumerate(consumed):
        mine = seen[first:upto]
        first = upto
        assert len(mine) == len(batches), "one fold per backward"
        sumsq = 0.0
        for i, p in enumerate(params):
            gs = [m[i] for m in mine if m[i] is not None]
            assert gs and accs[i] is not None and accs[i].dtype == torch.float32
            if p.dtype == torch.bfloat16:
                assert all(g.dtype == torch.bfloat16 for g in gs)
                want = seq_sum(gs)
            else:
                want = gs[-1]  # an fp32 p.grad is autograd's own running fp32 sum: its last sighting is the total
            assert torch.equal(bits(accs[i]), bits(want)), f"step {s + 1}, parameter {i}: the step did not consume the sequential fp32 sum"
            sumsq += math.fsum((want.double().flatten() ** 2).tolist())
        exact = math.sqrt(sumsq)
        assert abs(norms[s] - exact) <= 1e-6 * exact, (norms[s], exact)
    assert all(p.grad is None for p in params) and not opt._acc_filled


# ---- 5. two ranks on one GPU over gloo ----------------------------------------------------------------------------------------------------
RANK_SIZES = [5000, CHUNK + 3, 777]  # bf16, bf16, fp32 (bypasses the accumulator)
RANK_MICRO = 5


def _rank_params(torch_, dev):
    gen = torch_.Generator().manual_seed(0)
    dts = [torch_.bfloat16, torch_.bfloat16, torch_.float32]
    return [torch_.nn.Parameter((torch_.randn(n, generator=gen) * 0.05).to(device=dev, dtype=dt)) for n, dt in zip(RANK_SIZES, dts)]


def _rank_grads(rank):
    """[micro][param] CPU tensors or None.  Rank 1 never has a gradient for parameter 0 (an empty slot contributes zeros) and none for the
    fp32 parameter either."""
    rng = np.random.default_rng(500 + rank)
    dts = [torch.bfloat16, torch.bfloat16, torch.float32]
    out = []
    for k in range(RANK_MICRO):
        row = []
        for i, (n, dt) in enumerate(zip(RANK_SIZES, dts)):
            g = torch.from_numpy(log_uniform_grads(rng, n, 1)[0]).to(dt)
            row.append(None if (rank == 1 and i in (0, 2)) else g)
        out.append(row)
    return out


def _accum_worker(rank: int, world: int, port: int, out_q) -> None:
    try:
        import torch.distributed as dist

        from pipelinerl_amd.finetune.optim import FusedAdamW

        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        dev = torch.device("cuda", 0)
        torch.cuda.set_device(dev)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        params = _rank_params(torch, dev)
        opt = FusedAdamW(params, lr=1e-3, weight_decay=0.01, grad_accum_dtype=torch.float32)
        for row in _rank_grads(rank):
            for p, g in zip(params, row):
                if g is None:
                    continue
                if p.grad is None:
                    p.grad = g.to(dev)
                else:
                    p.grad += g.to(dev)
            opt.accumulate_grads()
        opt.reduce_accumulated(dist.group.WORLD)
        report = {"reduced": [opt._grad_of(p).detach().cpu().numpy() for p in params]}
        norm = opt.clip_and_step(0.05)
        report["norm"] = float(norm)
        report["params"] = [p.detach().float().cpu().numpy() for p in params]
        torch.cuda.synchronize(dev)
        dist.barrier()
        dist.destroy_process_group()
        out_q.put((rank, report))
    except Exception as e:  # noqa: BLE001
        import traceback

        out_q.put((rank, {"exception": f"{type(e).__name__}: {e}\n{traceback.format_exc()}"}))


def test_reduce_accumulated_two_ranks_over_gloo(libprl, cuda_device):
    import socket

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    procs = [ctx.Process(target=_accum_worker, args=(r, 2, port, q), daemon=True) for r in range(2)]
    for p in procs:
        p.start()
    try:
        results = dict(q.get(timeout=240) for _ in range(2))
    finally:
        status = []
        for p in procs:
            p.join(timeout=60)  # each child under its own limit
            if p.is_alive():
                p.kill()
                p.join(timeout=10)
            status.append(p.exitcode)
    for r in (0, 1):
        assert "exception" not in results[r], results[r]["exception"]
    assert status == [0, 0], f"exit status of the two ranks: {status}"
    # every rank's own sum, formed on the CPU from the gradients it was given; an absent gradient is zeros
    own = []
    for r in (0, 1):
        rows = _rank_grads(r)
        own.append([seq_sum([row[i] for row in rows]) if rows[0][i] is not None else torch.zeros(n) for i, n in enumerate(RANK_SIZES)])
    for i in range(len(RANK_SIZES)):
        want = (own[0][i] + own[1][i]) / 2
        a, b = torch.from_numpy(results[0]["reduced"][i]), torch.from_numpy(results[1]["reduced"][i])
        assert a.dtype == torch.float32 and torch.equal(bits(a), bits(b)), f"parameter {i}: the ranks hold different reduced gradients"
        assert torch.equal(bits(a), bits(want)), f"parameter {i}: not (acc_rank0 + acc_rank1) / 2"
    assert results[0]["norm"] == results[1]["norm"]
    start = _rank_params(torch, "cpu")
    for i, (pa, pb) in enumerate(zip(results[0]["params"], results[1]["params"])):
        assert np.array_equal(pa.view(np.uint32), pb.view(np.uint32)), f"parameter {i} differs between the ranks after the step"
        assert not np.array_equal(pa, start[i].detach().float().numpy()), "the step moved it (on rank 1 too, whose own slot was empty)"
