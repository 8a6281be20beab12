"""The value-head branch at the edges of its own kernels: `value_head_partial_kernel<float / bf16>` + `value_head_finalize_kernel`
through the C ABI `prl_value_head_fwd_bwd` (the launches here pass output buffers pre-filled with NaN, so an entry nobody wrote cannot
pass for a stale correct one), `value_head_terms` on top of it and `rl_step` with an actor-critic model on top of that.

Every entry of the advantages column is compared bit for bit, every entry of d value_loss / d value and every statistic with the fp64
witness of tests/value_term_checks.py under VALUE_GRAD_BOUND / VALUE_STAT_BOUND / VALUE_LOSS_BOUND (4 x the oracle's own fp32 error,
measured on the CPU by tests/test_value_term_checks_host.py on the cases built HERE); exact zeros and max / min exactly.

Paths no other test pins, and the case that reaches each:
  * cols = 1 (no pair at all), cols = 2 (one), one block more or less than full, [B, L] rows whose last column has no target and whose
    column 0 has no prediction, the second round of the grid-stride loop (more than 1024 x 256 entries), rows ending inside it;
    fp32 and bf16 predictions; group normalization x overlong filtering                                            (test_shapes)
  * the only labels at column 1, at column cols - 1, on both sides of every row start and segment boundary, in column 0 (ignored); an
    overflowed sequence, a sequence without labels, num_labels differing between neighbours                        (test_placement)
  * NaN, +inf, -inf, 3e19 on a labelled and on an unlabelled token, group_tokens == 0 under group normalization     (test_nonfinite)
  * nothing labelled: five zeros                                                                                   (test_no_labels)
  * two launches bit-identical, no gradient wanted: the same loss, advantages and statistics                       (inside test_shapes)
  * `rl_step`: d loss / d value through autograd with an upstream factor, fp32 and bf16 predictions, the policy term reading the
    value column; a NaN prediction on a labelled token                                                             (test_autograd, test_rl_step_nan)
"""

import ctypes
import functools
import types

import numpy as np
import pytest
import torch

import value_term_checks as vc

pytestmark = pytest.mark.gpu

F32 = np.float32
SHAPES = [(1, 1), (1, 2), (1, 255), (1, 256), (1, 257), (7, 64), (3, 1001), (1, 262144), (1, 262145), (3, 87383)]
ROUND = 1024 * 256  # entries of one round of the kernel's grid-stride loop (kMaxBlocks x kBlock of csrc/prl_value.hip)
WEIGHT_CFGS = [(gn, of) for gn in (False, True) for of in (False, True)]
PLACEMENT_SHAPES = [(1, 1001), (7, 64)]
NONFINITE_KINDS = ("nan", "plus_inf", "minus_inf", "3e19", "group_tokens_zero")
NONFINITE_SHAPES = [(1, 515), (3, 173)]
E2E_SHAPES = [(1, 1024), (3, 341)]
E2E_VOCAB, E2E_DIM = 256, 64
CASE_NAMES = ("shapes", "placement", "nonfinite", "e2e")


def value_cfg(gn=False, of=False, coef=0.25):
    return dict(policy_loss="ppo", epsilon_low=0.2, epsilon_high=0.2, kl_coef=0.0, final_kl_coef=0.0, batch_size=16, group_normalization=gn,
                overlong_filtering=of, value_loss_coef=coef, use_advantages=True, relu_log_p_weights=False, clamp_log_ratio_ref_new_value=10,
                temperature=1.0, divide_advantage_by_std=False)


def cfg_id(c):
    return f"gn{int(c['group_normalization'])}_of{int(c['overlong_filtering'])}"


def to_bf16(a):
    """Round to bfloat16 and back: the fp32 numbers the kernel sees of a bf16 prediction."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F32)).to(torch.bfloat16).float().numpy()


# ---- inputs (pure host code; tests/test_value_term_checks_host.py measures the oracle on the same arrays) --------------------
def edge_positions(rows, cols, starts):
    """Flat token positions that the issue wants labelled: column 1 and column cols - 1 of every row, column 0 of every row (a label
    there predicts nothing and must be ignored), both sides of every row start and of every segment start."""
    pos = set()
    for r in range(rows):
        pos.update(r * cols + c for c in (0, 1, cols - 1) if 0 <= c < cols)
    for s in starts:
        pos.update(p for p in (s - 1, s, s + 1) if 0 <= p < rows * cols)
    return np.asarray(sorted(pos), dtype=np.int64)


@functools.lru_cache(maxsize=None)
def build(rows, cols, seed=0, sparse=False):
    """(batch dict, value [rows, cols] fp32).  rows == 1: a packed row of sequences of 1 .. 8192 tokens; rows > 1: [B, L], one sequence
    per row.  Of three or more sequences, sequence 1 has no label at all and sequence 2 overflow = 1 (of two, sequence 1 overflow = 1); unlabelled tokens carry ordinary values, so a mask that fails
    shows.  `sparse`: the only labels are those of `edge_positions`."""
    rng = np.random.default_rng(1000003 * rows + cols + 7919 * seed + (500000 if sparse else 0))
    N = rows * cols
    if rows == 1:
        lens, left = [], cols
        top = max(1, min(8192, cols // 5))
        while left > 0:
            n = int(min(left, rng.integers(1, top + 1)))
            lens.append(n)
            left -= n
    else:
        lens = [cols] * rows
    lens = np.asarray(lens, dtype=np.int64)
    S = len(lens)
    start = np.concatenate([[0], np.cumsum(lens)[:-1]])
    sid = np.repeat(np.arange(S), lens)
    pos = np.arange(N) - start[sid]
    edges = edge_positions(rows, cols, start.tolist())
    if sparse:
        lab = np.zeros(N, dtype=bool)
    else:
        prompt = np.floor(lens * rng.uniform(0.1, 0.3, S)).astype(np.int64)
        lab = (pos >= prompt[sid]) & (rng.random(N) >= 0.05)
    lab[edges] = True
    if N > ROUND + 1:
        lab[ROUND + 1] = True  # the first entry of the second round of the grid-stride loop has a labelled target
    if S > 2:
        lab[sid == 1] = False  # a sequence without labels
    ids = rng.integers(3, E2E_VOCAB, size=N).astype(np.int64)
    n_lab = np.bincount(sid, weights=lab, minlength=S)
    ovf = np.zeros(S)
    if S > 1:
        ovf[2 if S > 2 else 1] = 1.0
    per_seq = lambda v: np.asarray(v, dtype=F32)[sid].reshape(rows, cols)  # noqa: E731
    batch = dict(
        labels=np.where(lab, ids, -100).reshape(rows, cols), input_ids=ids.reshape(rows, cols), attention_mask=np.ones((rows, cols), dtype=np.int64),
        rewards=per_seq(rng.choice([0.0, 0.25, 1.0, -0.5, 0.75], S)), group_tokens=per_seq(rng.integers(20, 5000, S)), num_labels=per_seq(n_lab),
        overflow=per_seq(ovf), old_logprobs=rng.normal(-5.5, 0.3, N).astype(F32).reshape(rows, cols),
        ref_logprobs=rng.normal(-5.5, 0.3, N).astype(F32).reshape(rows, cols), advantages=rng.normal(0, 1, N).astype(F32).reshape(rows, cols),
        model_version=0, is_packed=rows == 1)
    if rows == 1:
        batch.update(position_ids=pos.reshape(1, cols), segment_ids=sid.reshape(1, cols))
    value = (0.4 + 0.3 * rng.standard_normal(N)).astype(F32).reshape(rows, cols)
    return batch, value


def poisoned(kind, labelled, shape):
    """(batch, value, flat entry index) with one entry poisoned: its prediction NaN / +-inf / 3e19, or the group_tokens of its target 0;
    the target is labelled or not, the sequence neither overflowed nor the first of its row."""
    rows, cols = shape
    b, value = build(rows, cols, seed=11)
    lab = b["labels"].reshape(-1) != -100
    col = np.tile(np.arange(cols), rows)
    tgt_ok = (col >= 1) & (b["overflow"].reshape(-1) == 0) & (lab == labelled)
    i = int(np.flatnonzero(tgt_ok)[37 if labelled else 5]) - 1
    b = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in b.items()}
    value = value.copy()
    if kind == "group_tokens_zero":
        b["group_tokens"].reshape(-1)[i + 1] = 0.0
    else:
        value.reshape(-1)[i] = {"nan": np.nan, "plus_inf": np.inf, "minus_inf": -np.inf, "3e19": 3e19}[kind]
    return b, value, i


def no_label_batch(shape):
    b, value = build(*shape, seed=13)
    b = dict(b, labels=np.full_like(b["labels"], -100))
    return b, value


def e2e_model():
    from test_gpu_value_head import TinyActorCritic

    torch.manual_seed(31)
    model = TinyActorCritic(E2E_VOCAB, E2E_DIM)
    torch.nn.init.normal_(model.value_head.output.weight, std=0.3)
    return model


@functools.lru_cache(maxsize=None)
def e2e_host(shape, dtype):
    """The e2e batch with the critic's predictions computed on the host (the device's differ from them by the rounding of one
    64-term dot product; the GPU test hands the witness what the device produced)."""
    b, _ = build(*shape, seed=17)
    with torch.no_grad():
        v = e2e_model()(input_ids=torch.from_numpy(b["input_ids"])).value.float().numpy()
    return b, (to_bf16(v) if dtype == "bf16" else v)


def host_cases(name):
    """(label, loss config, batch, value as the device sees it) of every launch of a case: what the oracle is measured on."""
    out = []
    if name == "shapes":
        for rows, cols in SHAPES:
            b, v = build(rows, cols)
            for dtype in ("f32", "bf16"):
                vv = to_bf16(v) if dtype == "bf16" else v
                out += [(f"{rows}x{cols} {dtype} {cfg_id(value_cfg(gn, of))}", value_cfg(gn, of), b, vv) for gn, of in WEIGHT_CFGS]
    elif name == "placement":
        for rows, cols in PLACEMENT_SHAPES:
            b, v = build(rows, cols, seed=3, sparse=True)
            out += [(f"{rows}x{cols} {cfg_id(value_cfg(gn, of))}", value_cfg(gn, of), b, v) for gn, of in WEIGHT_CFGS]
    elif name == "nonfinite":
        for shape in NONFINITE_SHAPES:
            for kind in NONFINITE_KINDS:
                for labelled in (True, False):
                    b, v, _ = poisoned(kind, labelled, shape)
                    out += [(f"{shape} {kind} labelled={labelled} {cfg_id(c)}", c, b, v) for c in (value_cfg(True, True), value_cfg(False, False))]
            b, v = no_label_batch(shape)
            out.append((f"{shape} no labels", value_cfg(True, True), b, v))
    elif name == "e2e":
        for shape in E2E_SHAPES:
            for dtype in ("f32", "bf16"):
                b, v = e2e_host(shape, dtype)
                out.append((f"{shape} {dtype}", value_cfg(True, True), b, v))
    else:
        raise KeyError(name)
    return out


# ---- launches -------------------------------------------------------------------------------------------------------------------
def c_cfg_of(cfg):
    from pipelinerl_amd.finetune.rl import RLConfig, make_loss_config

    return make_loss_config(RLConfig(**cfg), 0, 10)[0]


def upload(batch, dev):
    d = {k: torch.from_numpy(np.ascontiguousarray(batch[k], dtype=F32)).to(dev) for k in ("rewards", "group_tokens", "num_labels", "overflow")}
    d["labels"] = torch.from_numpy(np.ascontiguousarray(batch["labels"])).to(dev)
    return d


def value_tensor(value, dtype, dev):
    """(device tensor handed to the kernel, the fp32 numbers it holds)."""
    t = torch.from_numpy(np.ascontiguousarray(value, dtype=F32)).to(dev)
    if dtype == "bf16":
        t = t.to(torch.bfloat16)
    return t, t.float().cpu().numpy()


def launch(lib, d, c_cfg, vt, want_grad=True):
    """`prl_value_head_fwd_bwd` as `value_head_terms` issues it, into NaN-filled outputs -> (value_loss_out fp32, advantages, statistics
    dict, d value or None), numpy."""
    from pipelinerl_amd import _lib
    from pipelinerl_amd.finetune.rl import _loss_workspace

    rows, cols = d["labels"].shape
    dev = vt.device
    nan32 = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device=dev)  # noqa: E731
    adv, g, vloss = nan32(rows, cols), (nan32(rows, cols) if want_grad else None), nan32(1)
    stats = torch.full((_lib.PRL_NUM_VALUE_STATS,), float("nan"), dtype=torch.float64, device=dev)
    ws = _loss_workspace(dev)
    with torch.cuda.device(dev):
        _lib.check(lib.prl_value_head_fwd_bwd(
            ctypes.byref(c_cfg), rows, cols, _lib.ptr(d["labels"]), _lib.ptr(vt), _lib.PRL_DTYPE_BF16 if vt.dtype == torch.bfloat16 else _lib.PRL_DTYPE_F32,
            _lib.ptr(d["rewards"]), _lib.ptr(d["group_tokens"]), _lib.ptr(d["num_labels"]), _lib.ptr(d["overflow"]), _lib.ptr(adv), _lib.ptr(g),
            _lib.ptr(vloss), _lib.ptr(stats), _lib.ptr(ws), ws.numel(), _lib.current_stream_ptr(dev)))
    torch.cuda.synchronize(dev)
    return (vloss.cpu().numpy()[0], adv.cpu().numpy(), dict(zip(vc.VALUE_STAT_KEYS, stats.cpu().tolist())), None if g is None else g.cpu().numpy())


def held(label, res, w):
    """Print every figure, then assert: advantages bit for bit, d value per entry, the statistics."""
    vloss, adv, stats, g = res
    n_adv, at = vc.check_advantages(adv, w)
    rs = vc.check_stats(stats, w, loss_out=vloss)
    rg = vc.check_grad(g, w) if g is not None else None
    print(f"[value] {label}: advantages {n_adv} entries differ; {rg if rg is not None else 'no gradient asked'} (bound {vc.VALUE_GRAD_BOUND:.1e}); "
          f"{rs} (bounds {vc.VALUE_STAT_BOUND:.1e} / {vc.VALUE_LOSS_BOUND:.1e})")
    assert n_adv == 0, f"{label}: advantages differ at {at}"
    assert rg is None or rg.ok(), f"{label}: {rg}"
    assert rs.ok(), f"{label}: {rs} got {stats} want {w.stats}"
    return rg, rs


def same_results(a, b):
    """Two launches' loss, advantages and statistics bit for bit (NaN against NaN equal)."""
    eq = lambda x, y: np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True)  # noqa: E731
    return eq(a[0], b[0]) and eq(a[1], b[1]) and all(eq(a[2][k], b[2][k]) for k in vc.VALUE_STAT_KEYS)


# ---- tests ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("rows,cols", SHAPES, ids=[f"{r}x{c}" for r, c in SHAPES])
def test_shapes(libprl, cuda_device, rows, cols, dtype):
    b, value = build(rows, cols)
    d = upload(b, cuda_device)
    vt, seen = value_tensor(value, dtype, cuda_device)
    assert dtype == "f32" or not np.array_equal(seen, value) or value.size < 3
    for k, (gn, of) in enumerate(WEIGHT_CFGS):
        cfg = value_cfg(gn, of)
        w = vc.witness(cfg, value=seen, **vc.columns(b))
        res = launch(libprl, d, c_cfg_of(cfg), vt)
        held(f"{rows}x{cols} {dtype} {cfg_id(cfg)}", res, w)
        if cols > 2:
            assert w.mask.any() and (w.scale > 0).any()
            assert not of or rows * cols < 5 or (w.mask & (w.w32 == 0)).any()  # the overflowed sequence: labelled, weight 0
        if k == 3:
            again = launch(libprl, d, c_cfg_of(cfg), vt)
            assert same_results(res, again) and np.array_equal(res[3], again[3]), "two launches differ"
            no_grad = launch(libprl, d, c_cfg_of(cfg), vt, want_grad=False)
            assert same_results(res, no_grad), "want_grad=False changes the loss, the advantages or the statistics"
    if rows * cols > ROUND:  # labelled pairs past the first round of the grid-stride loop, and a row end among them
        w = vc.witness(value_cfg(), value=seen, **vc.columns(b))
        # (1 x 262145 has the row's last column alone there: no pair, a gradient of 0 that has to be WRITTEN - the buffer held NaN)
        assert not w.paired[rows * cols - 1] and (rows == 1 or (w.scale[ROUND] > 0 and 2 * cols < ROUND < 3 * cols))


@pytest.mark.parametrize("rows,cols", PLACEMENT_SHAPES, ids=[f"{r}x{c}" for r, c in PLACEMENT_SHAPES])
def test_placement(libprl, cuda_device, rows, cols):
    from pipelinerl_amd.finetune.rl import value_head_terms
    from pipelinerl_amd.finetune.types import PipelineBatchEncoding

    b, value = build(rows, cols, seed=3, sparse=True)
    d = upload(b, cuda_device)
    vt, seen = value_tensor(value, "f32", cuda_device)
    pb = PipelineBatchEncoding(**{k: (torch.from_numpy(v) if isinstance(v, np.ndarray) else v) for k, v in b.items()}).to_device(cuda_device)
    for gn, of in WEIGHT_CFGS:
        cfg = value_cfg(gn, of)
        w = vc.witness(cfg, value=seen, **vc.columns(b))
        res = launch(libprl, d, c_cfg_of(cfg), vt)
        held(f"placement {rows}x{cols} {cfg_id(cfg)}", res, w)
        # the wrapper `rl_step` calls: the same launch
        vloss, adv, vstats, g = value_head_terms(c_cfg_of(cfg), pb, vt)
        assert same_results(res, (vloss.cpu().numpy(), adv.cpu().numpy(), dict(zip(vc.VALUE_STAT_KEYS, vstats.cpu().tolist())))) and np.array_equal(g.cpu().numpy(), res[3])


@pytest.mark.parametrize("labelled", [True, False], ids=["labelled", "unlabelled"])
@pytest.mark.parametrize("kind", NONFINITE_KINDS)
def test_nonfinite(libprl, cuda_device, kind, labelled):
    """One poisoned entry among ordinary ones.  On a labelled target: a NaN prediction gives value_max = value_min = NaN (reference
    rl/__init__.py:443-444, `value_predictions[masks_shifted].max()`), adds 0 to the sums and gets no gradient; +-inf and 3e19 saturate
    value_mse / value_loss at FLT_MAX (sum_sum's nan_to_num) and get no gradient; group_tokens == 0 is w = inf.  On an unlabelled one:
    only the advantages column shows it."""
    for shape in NONFINITE_SHAPES:
        b, value, i = poisoned(kind, labelled, shape)
        d = upload(b, cuda_device)
        vt, seen = value_tensor(value, "f32", cuda_device)
        for cfg in (value_cfg(True, True), value_cfg(False, False)):
            w = vc.witness(cfg, value=seen, **vc.columns(b))
            assert w.mask[i] == labelled
            res = launch(libprl, d, c_cfg_of(cfg), vt)
            held(f"nonfinite {shape} {kind} labelled={labelled} {cfg_id(cfg)}", res, w)
            if kind == "nan":
                assert np.isnan(res[1].reshape(-1)[i + 1]) and np.isnan(res[2]["value_max"]) == labelled and np.isnan(w.stats["value_min"]) == labelled
            if labelled and (kind != "group_tokens_zero" or cfg["group_normalization"]):
                assert not w.finite[i] and res[3].reshape(-1)[i] == 0


@pytest.mark.parametrize("shape", NONFINITE_SHAPES, ids=["packed", "padded"])
def test_no_labels(libprl, cuda_device, shape):
    b, value = no_label_batch(shape)
    vt, seen = value_tensor(value, "f32", cuda_device)
    w = vc.witness(value_cfg(True, True), value=seen, **vc.columns(b))
    res = launch(libprl, upload(b, cuda_device), c_cfg_of(value_cfg(True, True)), vt)
    held(f"no labels {shape}", res, w)
    assert list(res[2].values()) == [0.0] * 5 and res[0] == 0 and not res[3].any()


class Tap(torch.nn.Module):
    """The actor-critic model with its predictions kept (and cast, and optionally poisoned) where `rl_step` reads them."""

    def __init__(self, inner, dtype, poison=None):
        super().__init__()
        self.inner, self.value_head, self.dtype, self.poison = inner, inner.value_head, dtype, poison

    def forward(self, **kw):
        out = self.inner(input_ids=kw["input_ids"])
        v = out.value.to(self.dtype)
        if self.poison is not None:
            v = v.clone()
            v.view(-1)[self.poison] = float("nan")
        v.retain_grad()
        self.seen = v
        return types.SimpleNamespace(logits=out.logits, value=v)


def _pipeline_batch(b, dev):
    from pipelinerl_amd.finetune.types import PipelineBatchEncoding

    return PipelineBatchEncoding(**{k: (torch.from_numpy(v) if isinstance(v, np.ndarray) else v) for k, v in b.items()}).to_device(dev)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("shape", E2E_SHAPES, ids=["packed", "padded"])
def test_autograd(libprl, cuda_device, monkeypatch, shape, dtype):
    """`rl_step` with an actor-critic model: d loss / d value per entry = value_loss_coef x upstream x the witness's gradient, and the
    policy term reads the value column.  Two more fp32 products than the kernel's own gradient (coef x upstream, times the entry): the
    bound is VALUE_GRAD_BOUND + 2^-23; a bf16 prediction receives its gradient rounded to bf16 (8 significand bits: unit roundoff 2^-8
    of the entry) on top."""
    from pipelinerl_amd.finetune import rl
    from pipelinerl_amd.finetune.rl import RLConfig, rl_step

    b, _ = build(*shape, seed=17)
    cfg = value_cfg(True, True, coef=0.25)
    upstream = 1.7
    model = Tap(e2e_model().to(cuda_device), torch.bfloat16 if dtype == "bf16" else torch.float32)
    seen_adv = []
    orig = rl._with_advantages
    monkeypatch.setattr(rl, "_with_advantages", lambda batch, adv: (seen_adv.append(adv), orig(batch, adv))[1])
    pb = _pipeline_batch(b, cuda_device)
    loss, stats = rl_step(model, pb, 0, 10, RLConfig(**cfg))
    (loss * upstream).backward()
    seen = model.seen.detach().float().cpu().numpy()
    w = vc.witness(cfg, value=seen, **vc.columns(b))
    n_adv, at = vc.check_advantages(seen_adv[0].cpu().numpy(), w)
    assert len(seen_adv) == 1 and n_adv == 0, f"the policy term's advantages differ from rewards - V at {at}"
    lab = (b["labels"] != -100)
    lab[:, 0] = False
    assert stats["max_advantage"] == float(w.adv.reshape(lab.shape)[lab].max()) and stats["min_advantage"] == float(w.adv.reshape(lab.shape)[lab].min())
    got = model.seen.grad.float().cpu().numpy().astype(np.float64).reshape(-1) / (cfg["value_loss_coef"] * upstream)
    live = w.scale > 0
    fmt = 2.0 ** -8 if dtype == "bf16" else 0.0
    allowed = (vc.VALUE_GRAD_BOUND + 2.0 ** -23) * w.scale + fmt * np.abs(w.grad)
    err = np.abs(got - w.grad)
    worst = float((err[live] / w.scale[live]).max())
    print(f"[value] e2e {shape} {dtype}: d loss / d value {worst:.3e} of the entry's terms (bound {vc.VALUE_GRAD_BOUND + 2.0 ** -23:.1e}"
          f"{' + 2^-8 of the entry' if fmt else ''})")
    assert live.sum() > 100 and (err <= allowed).all() and not got[~live].any()
    rs = vc.check_stats({k: stats[k] for k in vc.VALUE_STAT_KEYS}, w)
    print(f"[value] e2e {shape} {dtype}: {rs}")
    assert rs.ok(), rs


def test_rl_step_nan(libprl, cuda_device):
    """A NaN prediction on a labelled token.  The reference asserts on the logits' log-probs and on the final loss only (rl/__init__.py:213,
    262, 386): the NaN advantage and the NaN value-loss element both go through sum_sum's nan_to_num as 0, the loss is finite, nothing
    raises, and the statistics that select (value_max / value_min, max_advantage / min_advantage) report NaN.  Pinned to the oracle."""
    from oracle import rl_loss as orl
    from pipelinerl_amd.finetune.rl import RLConfig, rl_step

    shape = E2E_SHAPES[0]
    b, _ = build(*shape, seed=17)
    cfg = value_cfg(True, True)
    lab = np.flatnonzero((b["labels"][0, 1:] != -100) & (b["overflow"][0, 1:] == 0))
    i = int(lab[11])
    model = Tap(e2e_model().to(cuda_device), torch.float32, poison=i)
    loss, stats = rl_step(model, _pipeline_batch(b, cuda_device), 0, 10, RLConfig(**cfg))
    loss.backward()
    with torch.no_grad():
        logits = model.inner(input_ids=torch.from_numpy(b["input_ids"]).to(cuda_device)).logits.float().cpu().numpy()
    seen = model.seen.detach().cpu().numpy()
    with np.errstate(all="ignore"):
        want = orl.rl_step(logits, b, cfg, 0, 10, True, value=seen)
    assert np.isnan(seen[0, i]) and np.isfinite(float(want["loss"])) and np.isfinite(loss.item())
    nan_keys = sorted(k for k, v in want["stats"].items() if np.isnan(v))
    assert nan_keys == ["max_advantage", "min_advantage", "value_max", "value_min"]
    assert sorted(k for k, v in stats.items() if np.isnan(v)) == nan_keys, {k: stats[k] for k in nan_keys}
    w = vc.witness(cfg, value=seen, **vc.columns(b))
    rs = vc.check_stats({k: stats[k] for k in vc.VALUE_STAT_KEYS}, w)
    assert rs.ok(), rs
    assert model.seen.grad[0, i].item() == 0 and abs(loss.item() - float(want["loss"])) <= 1e-4 * max(1.0, abs(float(want["loss"])))
