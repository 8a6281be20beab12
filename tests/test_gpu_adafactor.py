"""The fused Adafactor kernels (csrc/prl_adafactor.hip) and `FusedAdafactor` on the GPU.

Acceptance is per entry (tests/adafactor_checks.py): witness = transformers' Adafactor in fp64 on the CPU, reference = the same
class in fp32, every step started from the witness's state before it; an entry passes iff |k - wit| <= 4 r_ref scale.  The
kernels are checked the same way: each step is launched from the witness's state (rounded to the kernel's dtypes)."""

import copy
import ctypes
import io
import math

import numpy as np
import pytest
import torch

from adafactor_checks import HYPER, adafactor_record, adafactor_steps, check_step, clip_case_grads, log_uniform_grads

pytestmark = pytest.mark.gpu

GUARD, CANARY = 64, 1536.0  # elements in front of and behind every buffer; exact in bf16
F32, BF16 = torch.float32, torch.bfloat16
LR, WD, COEFS = 1e-3, 0.01, [1.0, 0.37, 0.0123]


def bf16_round(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float32)).to(BF16).float().numpy().astype(np.float64)


def geometry(libprl):
    g = [ctypes.c_int64() for _ in range(4)]
    assert libprl.prl_adafactor_geometry(*[ctypes.byref(x) for x in g]) == 0
    return tuple(x.value for x in g)  # band rows, tile columns, segments per group, elements per group


class Guarded:
    """`values` inside a buffer of canaries; `off` elements off the allocation's alignment."""

    def __init__(self, values, dtype, device, off=0):
        v = torch.from_numpy(np.ascontiguousarray(values, dtype=np.float32).ravel())
        self.n, self.lo = v.numel(), GUARD + off
        self.buf = torch.full((self.n + 2 * GUARD + off,), CANARY, dtype=dtype, device=device)
        self.view = self.buf[self.lo:self.lo + self.n]
        self.view.copy_(v.to(dtype))
        self.shape = np.shape(values)

    def ptr(self):
        return self.view.data_ptr()

    def intact(self):
        return bool((self.buf[:self.lo] == CANARY).all() and (self.buf[self.lo + self.n:] == CANARY).all())

    def numpy(self):
        return self.view.float().cpu().numpy().astype(np.float64).reshape(self.shape)


def inputs(shape, seed, grad_dtype=F32, param_dtype=F32, steps=3):
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    p0 = rng.normal(0.0, 0.05, n).astype(np.float32).reshape(shape)
    grads = [g.reshape(shape) for g in log_uniform_grads(rng, n, steps)]
    for g in grads:
        g.flat[::7] = 0.0  # exact zeros: eps1 alone keeps their squares away from 0
    if grad_dtype == BF16:
        grads = [bf16_round(g).astype(np.float32) for g in grads]
    if param_dtype == BF16:
        p0 = bf16_round(p0).astype(np.float32)
    return p0, grads


def launch(libprl, device, specs, record=None):
    """One prl_adafactor_step over `specs` (dicts: rec, param_dtype, grad_dtype, master, off, live, lr, wd); returns what the
    kernels left per spec (None for a skipped one) after checking every canary."""
    table = (_lib().PrlAdafactorSegment * len(specs))()
    held = []
    for seg, sp in zip(table, specs):
        rec = sp["rec"]
        before, shape = rec["before"], rec["g"].shape
        pdt, gdt, off = sp.get("param_dtype", F32), sp.get("grad_dtype", F32), sp.get("off", 0)
        bufs = {"p": Guarded(before["p"], pdt, device, off), "g": Guarded(rec["g"], gdt, device, off)}
        if sp.get("master"):
            bufs["master"] = Guarded(before["p"], F32, device, off)
        if len(shape) >= 2:
            bufs["exp_avg_sq_row"] = Guarded(before.get("exp_avg_sq_row", np.zeros(shape[:-1])), F32, device)
            bufs["exp_avg_sq_col"] = Guarded(before.get("exp_avg_sq_col", np.zeros(shape[:-2] + shape[-1:])), F32, device)
            seg.row, seg.col = bufs["exp_avg_sq_row"].ptr(), bufs["exp_avg_sq_col"].ptr()
            seg.rows, seg.cols = shape[-2:]
            seg.batch = int(np.prod(shape[:-2]))
        else:
            bufs["exp_avg_sq"] = Guarded(before.get("exp_avg_sq", np.zeros(shape)), F32, device, off)
            seg.v, seg.batch, seg.rows, seg.cols = bufs["exp_avg_sq"].ptr(), 1, 1, shape[0]
        seg.param, seg.grad = bufs["p"].ptr(), bufs["g"].ptr() if sp.get("live", True) else None
        seg.master = bufs["master"].ptr() if "master" in bufs else None
        seg.param_dtype, seg.grad_dtype = (1 if pdt == BF16 else 0), (1 if gdt == BF16 else 0)
        seg.step, seg.lr, seg.weight_decay = rec["step"], sp.get("lr", LR), sp.get("wd", WD)
        held.append(bufs)
    need = ctypes.c_size_t(0)
    _lib().check(libprl.prl_adafactor_workspace_bytes(table, len(specs), ctypes.byref(need)))
    ws = torch.full((need.value + 2 * GUARD,), 0x5A, dtype=torch.uint8, device=device)
    _lib().check(libprl.prl_adafactor_step(table, len(specs), HYPER["eps1"], HYPER["clip_threshold"], HYPER["decay_rate"],
                                           None if record is None else record.data_ptr(), ws.data_ptr() + GUARD, need.value,
                                           torch.cuda.current_stream(device).cuda_stream))
    torch.cuda.synchronize(device)
    assert bool((ws[:GUARD] == 0x5A).all() and (ws[GUARD + need.value:] == 0x5A).all()), "the workspace's canaries"
    out = []
    for sp, bufs in zip(specs, held):
        assert all(b.intact() for b in bufs.values()), f"canaries around the buffers of {sp['rec']['g'].shape}"
        if not sp.get("live", True):
            for k, b in bufs.items():
                if k != "g":
                    want = sp["rec"]["before"].get(k if k != "master" else "p", np.zeros(b.shape))
                    assert np.array_equal(b.numpy(), Guarded(want, b.buf.dtype, "cpu").numpy()), "a segment without a gradient is untouched"
            out.append(None)
            continue
        got = {k: b.numpy() for k, b in bufs.items() if k not in ("g", "p", "master")}
        got["p"] = bufs["master" if "master" in bufs else "p"].numpy()
        if "master" in bufs:
            assert torch.equal(bufs["p"].view.view(torch.int16), bufs["master"].view.to(BF16).view(torch.int16)), "bf16 parameter = RNE(master)"
        assert np.array_equal(bufs["g"].numpy(), Guarded(sp["rec"]["g"], bufs["g"].buf.dtype, "cpu").numpy()), "the gradient is not rewritten"
        out.append(got)
    return out


def _lib():
    from pipelinerl_amd import _lib as lib

    return lib


def check_shape(libprl, device, shape, seed, name, off=0, wd=WD, **dtypes):
    p0, grads = inputs(shape, seed, dtypes.get("grad_dtype", F32), dtypes.get("param_dtype", F32))
    no_master = dtypes.get("param_dtype", F32) == BF16 and not dtypes.get("master")
    for rec in adafactor_steps(p0, grads, COEFS, LR, wd, p_round=bf16_round if no_master else None):
        record = torch.tensor([0.0, rec["coef"]], dtype=F32, device=device)
        got, = launch(libprl, device, [dict(rec=rec, off=off, wd=wd, **dtypes)], record)
        # without master weights the stored parameter is the bf16 image of the result: half a bf16 ulp of it on top of the bound
        extra = 2.0 ** (np.floor(np.log2(np.maximum(np.abs(rec["wit"]["p"]), 1e-300))) - 8) if no_master else None
        check_step(f"{name} {shape} step {rec['step']}", got, rec, extra_abs=extra)


def edge_shapes(libprl):
    band, tile, _, _ = geometry(libprl)
    shapes = [(1, 300), (300, 1), (1, 1), (67, 129), (64, 128), (2 * band + 3, tile + 5), (2, 3, 65)]  # 3 bands (not a power of two) x 2 tiles
    shapes += [(r, 24) for r in (band - 1, band, band + 1)] + [(5, c) for c in (tile - 1, tile, tile + 1)]
    shapes += [(n,) for n in (16383, 16384, 16385, band * tile - 1, band * tile, band * tile + 1, tile - 1, tile + 1)]
    return shapes


def test_edges_by_direct_abi_calls(libprl, cuda_device):
    for i, shape in enumerate(edge_shapes(libprl)):
        check_shape(libprl, cuda_device, shape, 100 + i, "fp32")
    for i, shape in enumerate([(67, 129), (64, 128), (1001,)]):  # a view one element off 16-byte alignment
        check_shape(libprl, cuda_device, shape, 200 + i, "fp32 unaligned view", off=1)


@pytest.mark.parametrize("case", ["bf16_master", "bf16_param_fp32_grad", "bf16_no_master", "fp32_param_bf16_grad"])
def test_dtypes(libprl, cuda_device, case):
    band, tile, _, _ = geometry(libprl)
    dtypes = {"bf16_master": dict(param_dtype=BF16, grad_dtype=BF16, master=True), "bf16_param_fp32_grad": dict(param_dtype=BF16, grad_dtype=F32, master=True),
              "bf16_no_master": dict(param_dtype=BF16, grad_dtype=BF16), "fp32_param_bf16_grad": dict(grad_dtype=BF16)}[case]
    for i, shape in enumerate([(67, 129), (64, 128), (band + 1, tile + 8), (2, 3, 65), (16385,), (300,)]):
        check_shape(libprl, cuda_device, shape, 300 + i, case, **dtypes)
    check_shape(libprl, cuda_device, (64, 128), 310, case + " unaligned view", off=1, **dtypes)


def test_table_longer_than_a_launch_with_holes(libprl, cuda_device):
    _, _, group_segments, _ = geometry(libprl)
    shapes = [(3, 5), (7,), (2, 2, 3), (65,), (1, 9)]
    specs = []
    for i in range(group_segments + 1 + 2):
        shape = shapes[i % len(shapes)]
        p0, grads = inputs(shape, 400 + i, steps=2)
        rec = adafactor_steps(p0, grads, [0.5, 0.5], LR, WD)[1]  # step 2: the state is not zero
        specs.append(dict(rec=rec, live=i != 11, param_dtype=BF16 if i % 3 == 0 else F32, master=i % 3 == 0))
    empty = {"before": {"p": np.zeros((0, 4))}, "g": np.zeros((0, 4), np.float32), "step": 1, "coef": 0.5}
    specs.insert(20, dict(rec=empty))  # numel == 0
    assert sum(sp.get("live", True) and sp["rec"]["g"].size > 0 for sp in specs) == group_segments + 2
    record = torch.tensor([0.0, 0.5], dtype=F32, device=cuda_device)
    for sp, got in zip(specs, launch(libprl, cuda_device, specs, record)):
        if got is not None and sp["rec"]["g"].size:
            check_step(f"table {sp['rec']['g'].shape}", got, sp["rec"])


@pytest.mark.parametrize("kind", ["below", "above"])
def test_update_clip_both_sides(libprl, cuda_device, kind):
    for shape in [(67, 129), (1000,)]:
        rng = np.random.default_rng(77)  # (the seeds and gradients of tests/test_adafactor_checks_host.py, which checks the ratios on the CPU)
        p0 = rng.normal(0.0, 0.05, shape).astype(np.float32)
        recs = adafactor_steps(p0, clip_case_grads(kind, rng, shape), [1.0] * 3, LR, WD)
        for rec in recs:
            if rec["step"] > 1:
                assert (rec["ratio"] < 1.0 - 1e-3) if kind == "below" else (rec["ratio"] > 1.0 + 1e-3)
            got, = launch(libprl, cuda_device, [dict(rec=rec)])
            check_step(f"update clip {kind} {shape} step {rec['step']} (rms / clip = {rec['ratio']:.4f})", got, rec)


# ---- FusedAdafactor -------------------------------------------------------------------------------------------------------
PARAM_SHAPES = [(67, 129), (64, 128), (2, 3, 65), (1000,), (1, 300), (5,)]


def make_params(device, seed, dtype=F32, grad_scale=1.0):
    params, p0s, grads = [], [], []
    for i, shape in enumerate(PARAM_SHAPES):
        p0, g = inputs(shape, seed + i, grad_dtype=dtype, param_dtype=dtype, steps=1)
        params.append(torch.nn.Parameter(torch.from_numpy(p0).to(device=device, dtype=dtype)))
        p0s.append(p0)
        grads.append((g[0] * grad_scale).astype(np.float32) if dtype == F32 else bf16_round(g[0] * grad_scale).astype(np.float32))
    return params, p0s, grads


def state_of(opt, p):
    st = opt.state[p]
    got = {k: st[k].float().cpu().numpy().astype(np.float64) for k in ("exp_avg_sq_row", "exp_avg_sq_col", "exp_avg_sq") if k in st}
    got["p"] = (st["master"] if "master" in st else p.detach()).float().cpu().numpy().astype(np.float64)
    return got


def groups(params):
    return [{"params": params[0::2], "weight_decay": WD}, {"params": params[1::2], "weight_decay": 0.0}]


@pytest.mark.parametrize("max_norm", [0.05, 1e6])
def test_clip_and_step_is_the_witness_fed_the_clipped_gradient(libprl, cuda_device, max_norm):
    from pipelinerl_amd.finetune.optim import FusedAdafactor

    runs = []
    for _ in range(2):
        params, p0s, grads = make_params(cuda_device, 500)
        opt = FusedAdafactor(groups(params), lr=LR)
        for p, g in zip(params, grads):
            p.grad = torch.from_numpy(g).to(cuda_device)
        norm = opt.clip_and_step(max_norm)
        runs.append((params, opt, float(opt._record[1])))
    params, opt, coef = runs[0]
    exact = math.sqrt(math.fsum(float((g.astype(np.float64) ** 2).sum()) for g in grads))
    assert abs(float(norm) - exact) <= 1e-6 * exact and (coef < 1.0) == (max_norm < exact)
    for i, (p, p0, g) in enumerate(zip(params, p0s, grads)):
        assert torch.equal(p.grad.cpu(), torch.from_numpy(g)), "clip_and_step leaves the gradients as they were"
        rec = adafactor_record({"p": p0}, g, coef, 1, LR, WD if i % 2 == 0 else 0.0)
        check_step(f"clip_and_step({max_norm}) {p0.shape}", state_of(opt, p), rec)
        twin = runs[1][0][i]
        assert torch.equal(p.detach().view(torch.int32), twin.detach().view(torch.int32)), "two identical runs are bitwise equal"
        for k, v in opt.state[p].items():
            assert torch.equal(v.cpu(), runs[1][1].state[twin][k].cpu()), k


def test_fp32_accumulation_of_300_micro_batches(libprl, cuda_device):
    from pipelinerl_amd.finetune.optim import FusedAdafactor

    params, p0s, grads = make_params(cuda_device, 600, dtype=BF16)
    opt = FusedAdafactor(groups(params), lr=LR, grad_accum_dtype=F32)
    for _ in range(300):
        for p, g in zip(params, grads):
            p.grad = torch.from_numpy(g).to(device=cuda_device, dtype=BF16)
        opt.accumulate_grads()
    opt.clip_and_step(None)
    for i, (p, p0, g) in enumerate(zip(params, p0s, grads)):
        total = np.zeros_like(g)
        for _ in range(300):
            total = total + g  # the sequential fp32 sum the accumulator holds
        rec = adafactor_record({"p": p0}, total, 1.0, 1, LR, WD if i % 2 == 0 else 0.0)
        check_step(f"fp32 accumulation {p0.shape}", state_of(opt, p), rec)
        assert p.grad is None


def test_state_exchange_with_transformers(libprl, cuda_device):
    from transformers.optimization import Adafactor

    from pipelinerl_amd.finetune.optim import FusedAdafactor

    rng = np.random.default_rng(700)
    params, p0s, _ = make_params(cuda_device, 700)
    G = [[g.reshape(s) for g in log_uniform_grads(rng, int(np.prod(s)), 3)] for s in PARAM_SHAPES]
    lib_opt = Adafactor(groups(params), lr=LR, relative_step=False, scale_parameter=False)
    for s in range(2):
        for p, g in zip(params, G):
            p.grad = torch.from_numpy(g[s]).to(cuda_device)
        lib_opt.step()
    before = [{"p": p.detach().cpu().numpy(), **{k: v.cpu().numpy() for k, v in lib_opt.state[p].items() if k.startswith("exp_avg_sq")}} for p in params]
    # transformers -> fused -> one step = the witness continued
    fused = FusedAdafactor(groups(params), lr=123.0)
    fused.load_state_dict(copy.deepcopy(lib_opt.state_dict()))
    assert fused.param_groups[0]["lr"] == LR and all("RMS" not in st for st in fused.state.values())
    for p, g in zip(params, G):
        p.grad = torch.from_numpy(g[2]).to(cuda_device)
    fused.step()
    recs = [adafactor_record(b, g[2], 1.0, 3, LR, WD if i % 2 == 0 else 0.0) for i, (b, g) in enumerate(zip(before, G))]
    for p, rec in zip(params, recs):
        assert float(fused.state[p]["step"]) == 3.0
        check_step(f"transformers -> fused {rec['g'].shape}", state_of(fused, p), rec)
    # torch.save / load round trip of the fused state, and fused -> transformers: step 4 from the fused state
    blob = io.BytesIO()
    torch.save(fused.state_dict(), blob)
    blob.seek(0)
    sd = torch.load(blob, weights_only=False)
    before = [state_of(fused, p) for p in params]
    g4 = [log_uniform_grads(rng, int(np.prod(s)), 1)[0].reshape(s) for s in PARAM_SHAPES]
    twins = [torch.nn.Parameter(p.detach().clone()) for p in params]
    again, back = FusedAdafactor(groups(twins), lr=LR), Adafactor(groups(params), lr=LR, relative_step=False, scale_parameter=False)
    again.load_state_dict(sd)
    back.load_state_dict({"state": {i: {k: v for k, v in st.items() if k != "master"} for i, st in sd["state"].items()}, "param_groups": sd["param_groups"]})
    for p, t, g in zip(params, twins, g4):
        p.grad, t.grad = torch.from_numpy(g).to(cuda_device), torch.from_numpy(g).to(cuda_device)
    again.step()
    back.step()
    for i, (p, t, b, g) in enumerate(zip(params, twins, before, g4)):
        rec = adafactor_record(b, g, 1.0, 4, LR, WD if i % 2 == 0 else 0.0)
        check_step(f"saved and loaded fused state {g.shape}", state_of(again, t), rec)
        got = {"p": p.detach().cpu().numpy(), **{k: v.cpu().numpy() for k, v in back.state[p].items() if k.startswith("exp_avg_sq")}}
        check_step(f"fused -> transformers {g.shape}", got, rec)


def test_master_weights_keep_updates_that_bf16_rounds_away(libprl, cuda_device):
    from transformers.optimization import Adafactor

    from pipelinerl_amd.finetune.optim import FusedAdafactor

    rng = np.random.default_rng(800)
    shape, steps, lr = (96, 160), 10, 1e-5  # |u| ~ 1: an update of ~1e-5 is below half a bf16 ulp (1.2e-4) of weights in [0.05, 0.06]
    p0 = torch.from_numpy((0.05 + 0.01 * rng.random(shape)).astype(np.float32)).to(BF16)
    grads = [torch.from_numpy(rng.uniform(0.5, 1.5, shape).astype(np.float32)).to(BF16) for _ in range(steps)]  # |u| ~ 1 on every entry
    stock = torch.nn.Parameter(p0.clone().to(cuda_device))
    so = Adafactor([stock], lr=lr, relative_step=False, scale_parameter=False)
    p = torch.nn.Parameter(p0.clone().to(cuda_device))
    opt = FusedAdafactor([p], lr=lr, master_weights=True)
    for g in grads:
        stock.grad, p.grad = g.to(cuda_device), g.to(cuda_device)
        so.step()
        opt.step()
    unchanged = (stock.detach().cpu().view(torch.int16) == p0.view(torch.int16)).float().mean().item()
    print(f"[adafactor] transformers.Adafactor on the bf16 parameter, lr {lr}, {steps} steps: {unchanged:.2%} of the entries never moved")
    assert unchanged > 0.99, "transformers' Adafactor on the bf16 parameter loses the updates"
    master = opt.state[p]["master"]
    assert torch.equal(p.detach().view(torch.int16), master.to(BF16).view(torch.int16))
    moved = (master.cpu() < p0.float()).float().mean().item()
    assert moved > 0.99, f"the master copy carries the updates the bf16 parameter cannot ({moved:.2%} moved against the positive gradients)"


def test_learner_step_matches_transformers_adafactor(libprl, cuda_device, tmp_path):
    from test_gpu_optim import TinyLM

    from pipelinerl_amd import streams
    from pipelinerl_amd.finetune.optim import FusedAdafactor, get_optimizer
    from pipelinerl_amd.finetune.rl import RLConfig
    from pipelinerl_amd.finetune_loop import TRAINER_TOPIC, LearnerStep
    from pipelinerl_amd.hotpath import HotPathStep, dense_micro_batches
    from pipelinerl_amd.synthetic import make_ragged

    V, thr = 128, 0.05
    rag_h, _ = make_ragged(4, attempts=4, seq_length=40, vocab=V, seed=3, prompt_min=3, prompt_max=8, with_ref=True)
    mbs = dense_micro_batches(rag_h, 100)
    rl = RLConfig(policy_loss="ppo", epsilon_low=0.2, epsilon_high=0.2, kl_coef=0.05, final_kl_coef=0.05, divide_advantage_by_std=True,
                  clamp_log_ratio_ref_new_value=5)
    cfg = rl.model_copy()
    cfg.batch_size = 16
    batches = HotPathStep(cfg, 2, 0, 10).preprocess(rag_h.to(cuda_device), mbs)
    torch.manual_seed(0)
    models = [TinyLM(V).to(cuda_device)]
    models.append(copy.deepcopy(models[0]))
    names = [n for n, _ in models[0].named_parameters()]
    p0 = [p.detach().cpu().numpy().copy() for p in models[0].parameters()]
    opts = [get_optimizer("adafactor_hip", models[0], LR, WD), get_optimizer("adafactor", models[1], LR, WD)]
    assert isinstance(opts[0], FusedAdafactor) and hasattr(opts[0], "clip_and_step") and not hasattr(opts[1], "clip_and_step")
    norms, seen = [], []
    for k, (model, opt) in enumerate(zip(models, opts)):
        streams.reset_streams_backend()
        streams.set_streams_backend("files")
        if k == 0:  # the gradients the fused step consumed, for the witness
            zero = opt.zero_grad
            opt.zero_grad = lambda *a, _z=zero, _m=model, **kw: seen.append([p.grad.detach().cpu().numpy().copy() for p in _m.parameters()]) or _z(*a, **kw)
        (tmp_path / f"run{k}").mkdir(exist_ok=True)
        step = LearnerStep(model, opt, rl, train_batch_size=1, gradient_accumulation_passes=16, max_train_steps=10, send_weight_updates=False,
                           gradient_clipping_threshold=thr, trainer_stream=streams.SingleStreamSpec(exp_path=tmp_path / f"run{k}", topic=TRAINER_TOPIC))
        for i, b in enumerate(batches):
            assert step.step(b)["did_optimizer_step"] == (i == len(batches) - 1)
        norms.append(step.metrics.grad_norm)
    streams.reset_streams_backend()
    assert len(seen) == 1 and abs(norms[0] - norms[1]) <= 1e-6 * norms[1]
    coef = float(np.float32(thr) / (np.float32(norms[0]) + np.float32(1e-6))) if norms[0] > thr else 1.0
    for name, a, b, p, g in zip(names, models[0].parameters(), models[1].parameters(), p0, seen[0]):
        rec = adafactor_record({"p": p}, g, coef, 1, LR, 0.0 if "bias" in name else WD)
        check_step(f"LearnerStep + adafactor_hip {name}", state_of(opts[0], a), rec)
        check_step(f"LearnerStep + clip_grad_norm_ + transformers.Adafactor {name}", {"p": b.detach().cpu().numpy(), **{k: v.cpu().numpy() for k, v in opts[1].state[b].items() if k.startswith("exp_avg_sq")}}, rec)
