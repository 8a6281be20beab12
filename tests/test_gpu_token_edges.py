"""The token-level loss term (`policy_loss` "ppo" / "reinforce") at the edges of its own kernel: `grpo_loss_partial_kernel`
<VEC = 4 / 2 / 1, FAST> + `grpo_loss_finalize_kernel` through the C ABI `prl_grpo_loss_fwd_bwd` (what `grpo_loss_from_logprobs`
calls; the launches here pass output buffers pre-filled with NaN, so an entry nobody wrote cannot pass for a stale correct one),
and `rl_step` in both modes on top.

Every token's g_nlp / g_ent and every statistic is compared with the fp64 witness of tests/token_term_checks.py under TOKEN_BOUND /
STAT_BOUND / LOSS_BOUND (4 x the oracle's own fp32 error, measured on the CPU by tests/test_token_term_checks_host.py on the cases
built HERE); exact zeros, counts, counters and max / min exactly.

Paths no other test pins, and the case that reaches each:
  * the four PPO quadrants, a zero / negative-zero advantage, the REINFORCE clamp, the KL clamp exactly at +-C and outside, relu with
    A < 0, rewards as weights, group normalization, overflow = 1 under filtering, the entropy term - as a table      (test_branches)
  * epsilon = 0 and new == old: the ratio on both bounds, min() ties                                                (test_exact_tie)
  * NaN / inf advantage, ratio = inf on either side of min(), ratio^2 overflowing, NaN entropy, num_labels 0 / 0.5  (test_nonfinite)
  * VEC = 4 FAST, VEC = 2 FAST (statistics only), VEC = 1 branchy on misaligned views, T % 4 tails; bit-equal gradients (test_paths)
  * the second and third round of the software-pipelined grid-stride loop, a ragged last round, flat micro-batches  (test_rounds)
  * padded [B, L]: the in-group column wrap, column 0 of every row, L = 1, padding with num_labels = group_tokens = 0 (test_padded)
  * position_ids == 0 at each slot of a 4-token group, at the first / last group of a block's span, at token 0      (test_flat_starts)
  * the clip branches inside the fused logits kernel's `prl_token_grad`                                             (test_end_to_end)
"""

import ctypes
import functools
import itertools
import types

import numpy as np
import pytest
import torch

import grad_checks as gc
import token_term_checks as tc

pytestmark = pytest.mark.gpu

F32 = np.float32
RATIOS = (0.90, 0.97, 1.0, 1.03, 1.10)   # at epsilon = 0.05: every one at least 2 % from the clip bounds 0.95 / 1.05
KL_TABLE = (-2.0, -1.0, 0.0, 1.0, 2.0)   # ref - new in units of C: outside, exactly on -C, inside, exactly on C, outside
ADV_CLASSES = 4                          # > 0, < 0, 0.0, -0.0
ROUNDS_T = 2 * 2048 * 256 * 4 + 5 * 1024 + 3  # two whole rounds of the largest possible grid at 4 tokens per lane, a ragged third, a % 4 tail
E2E_T, E2E_V = 600, 1031


def loss_cfg(policy="ppo", relu=False, use_adv=True, gn=False, of=False, ent=False, eps=0.05, C=1.0, kl=0.05):
    e = 0.01 if ent else 0.0
    return dict(policy_loss=policy, epsilon_low=eps, epsilon_high=eps, kl_coef=kl, final_kl_coef=kl, batch_size=16, group_normalization=gn,
                overlong_filtering=of, relu_log_p_weights=relu, use_advantages=use_adv, clamp_log_ratio_ref_new_value=C, entropy_bonus=e,
                final_entropy_bonus=e, divide_advantage_by_std=False)


def cfg_id(c):
    return (f"{c['policy_loss']}_relu{int(c['relu_log_p_weights'])}_adv{int(c['use_advantages'])}_gn{int(c['group_normalization'])}"
            f"_of{int(c['overlong_filtering'])}_ent{int(c['entropy_bonus'] != 0)}_eps{c['epsilon_low']}")


# the product of the switches; the reference can express every combination of it, so none is skipped
BRANCH_CFGS = [loss_cfg(p, r, a, g, o, e) for p, r, a, g, o, e in itertools.product(("ppo", "reinforce"), (False, True), (True, False),
                                                                                   (False, True), (False, True), (False, True))]
TIE_CFGS = [loss_cfg(eps=0.0, ent=True), loss_cfg(eps=0.0, gn=True, of=True)]
ROUNDS_CFG = loss_cfg(gn=True, of=True, ent=True, C=0.1)
PADDED_CFG = loss_cfg(ent=True, C=0.1)
FLAT_CFG = loss_cfg(gn=True, ent=True, C=0.1)
NF_CFG = loss_cfg(ent=True, C=0.1)
E2E_CFG = loss_cfg(ent=True)


# ---- inputs (pure host code; tests/test_token_term_checks_host.py measures the oracle on the same arrays) --------------------
def build_packed(lens, seed, *, table=False, tie=False, C=0.1, new=None, entropy=None, overflow_share=0.1):
    """The columns of one packed row ([1, T] numpy).  Sequences of `lens` tokens: a prompt of 10 .. 30 % without labels, 5 % of the
    rest unlabelled observation tokens; unlabelled tokens carry ordinary values too, so a mask that fails shows.
    `table`: ratio target, advantage class and ref - new walk through RATIOS x 4 x KL_TABLE by token index, new log-probs are
    multiples of 0.25 so that ref - new = +-C, +-2C is exact (C must be a multiple of 0.25); otherwise they are drawn: ratio targets
    from RATIOS with 0.4 % jitter (exactly 1 for a fifth); |ref - new| exactly 0 for 10 %, in 0.2 .. 0.8 C for 80 %, in 1.5 .. 3 C for the
    rest.  Nothing in (0, 0.2 C): the metric's KL scale |kl_coef| |1 - e^cl| is itself a difference, good to 2^-24 / |cl| only, and at
    |cl| -> 0 the fp32 reference is off by half the term (measured: 0.5 at |cl| ~ 1e-7) - no yardstick there.
    `tie`: new == old everywhere.  `new` / `entropy` [T]: log-probs and entropies given from outside (a model's)."""
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, dtype=np.int64)
    S, T = len(lens), int(lens.sum())
    start = np.concatenate([[0], np.cumsum(lens)[:-1]])
    sid = np.repeat(np.arange(S), lens)
    pos = np.arange(T) - start[sid]
    prompt = np.floor(lens * rng.uniform(0.1, 0.3, S)).astype(np.int64)
    lab = (pos >= prompt[sid]) & (rng.random(T) >= 0.05)
    ids = rng.integers(0, E2E_V, size=T).astype(np.int64)
    labels = np.where(lab, ids, -100)
    idx = np.arange(T)
    if new is None:
        new = (-0.25 * rng.integers(1, 13, T)).astype(F32) if table else rng.uniform(-3.0, -0.05, T).astype(F32)
    else:
        new = np.asarray(new, dtype=F32)
    if table:
        r = np.asarray(RATIOS)[idx % 5]
        cls = (idx // 5) % ADV_CLASSES
        t = np.asarray(KL_TABLE)[(idx // 20) % 5] * C
    else:
        k = rng.integers(0, 5, T)
        r = np.asarray(RATIOS)[k] * np.where(k == 2, 1.0, 1.0 + rng.uniform(-0.004, 0.004, T))
        cls = rng.choice(ADV_CLASSES, size=T, p=[0.45, 0.45, 0.05, 0.05])
        where = rng.random(T)
        t = rng.choice([-1.0, 1.0], T) * np.select([where < 0.1, where < 0.9], [0.0, rng.uniform(0.2, 0.8, T)], rng.uniform(1.5, 3.0, T)) * C
    old = np.where((r == 1.0) | tie, new, (new.astype(np.float64) - np.log(r)).astype(F32)).astype(F32)
    ref = (new.astype(np.float64) + t).astype(F32)
    mag = rng.uniform(0.2, 2.0, T)
    adv = np.select([cls == 0, cls == 1, cls == 2], [mag, -mag, 0.0], -0.0).astype(F32)
    n_lab = np.bincount(sid, weights=lab, minlength=S)
    per_seq = lambda v: np.asarray(v, dtype=F32)[sid]  # noqa: E731
    batch = dict(
        labels=labels, input_ids=ids, position_ids=pos, segment_ids=sid, new_logprobs=new,
        entropy=rng.uniform(0.5, 3.0, T).astype(F32) if entropy is None else np.asarray(entropy, dtype=F32), old_logprobs=old, ref_logprobs=ref,
        advantages=adv, rewards=per_seq(rng.uniform(-1.0, 1.0, S)), group_tokens=per_seq(rng.integers(20, 5000, S)),
        num_labels=per_seq(np.maximum(n_lab, 1)), overflow=per_seq(rng.random(S) < overflow_share))
    batch = {k: v[None] for k, v in batch.items()}
    batch.update(attention_mask=np.ones((1, T), dtype=np.int64), model_version=0, is_packed=True)
    return batch


@functools.lru_cache(maxsize=None)
def branches_batch():
    rng = np.random.default_rng(201)
    return build_packed(rng.integers(30, 200, 24), 202, table=True, C=1.0, overflow_share=0.5)


@functools.lru_cache(maxsize=None)
def tie_batch():
    rng = np.random.default_rng(203)
    return build_packed(rng.integers(5, 120, 12), 204, tie=True, C=1.0, overflow_share=0.3)


@functools.lru_cache(maxsize=None)
def rounds_batch():
    rng = np.random.default_rng(205)
    lens = []
    left = ROUNDS_T
    while left > 0:
        n = int(min(left, rng.integers(1, 8193)))
        lens.append(n)
        left -= n
    lens[3], lens[4] = lens[3] + lens[4] - 1, 1  # a sequence of one token for certain
    return build_packed(lens, 206, C=0.1)


def padded_batch(B, L, side):
    """[B, L] as pad_collate writes it: rows of 0 .. L tokens, right- or left-padded; padding carries labels -100 and zeros in every
    RL column (num_labels = group_tokens = 0).  Every right-padded row labels its column 0, which predicts nothing."""
    rng = np.random.default_rng(1000 * B + L + (500000 if side == "left" else 0))
    n = rng.integers(0, L + 1, B)
    n[rng.integers(0, B)] = L
    if B > 2:
        n[1], n[2] = max(n[1], 1), 0
    row = build_packed(np.maximum(n, 1), 207 + B + L, C=0.1)
    out = {}
    starts = np.concatenate([[0], np.cumsum(np.maximum(n, 1))[:-1]])
    for k, v in row.items():
        if not isinstance(v, np.ndarray) or k in ("segment_ids", "position_ids"):
            continue
        fill = -100 if k == "labels" else 0
        a = np.full((B, L), fill, dtype=v.dtype)
        for b in range(B):
            if n[b]:
                sl = slice(0, n[b]) if side == "right" else slice(L - n[b], L)
                a[b, sl] = v[0, starts[b]:starts[b] + n[b]]
        out[k] = a
    for b in range(B):
        if side == "right" and n[b]:
            out["labels"][b, 0] = out["input_ids"][b, 0]
    out.update(model_version=0, is_packed=False)
    return out


PADDED_SHAPES = [(B, L, side) for L in (1, 2, 3, 5, 7, 1023, 1025) for B in (1, 2, 3, 257) for side in ("right", "left")]
FLAT_T = 8 * 1024 + 3


def flat_starts():
    """token 0; each slot of a 4-token group at the first and at the last group of a block's span of 256 lanes x 4 tokens; a group
    in mid-span with two starts; the last token."""
    s = {0, FLAT_T - 1}
    for slot in range(4):
        s |= {1024 * (slot + 1) + slot, 1024 * (slot + 1) + 1020 + (3 - slot)}
    s |= {5 * 1024 + 512, 5 * 1024 + 514, 6 * 1024 + 1, 6 * 1024 + 2}
    return np.asarray(sorted(s))


@functools.lru_cache(maxsize=None)
def flat_batch():
    st = flat_starts()
    lens = np.diff(np.concatenate([st, [FLAT_T]]))
    b = build_packed(lens, 208, C=0.1)
    b["labels"][0, st] = b["input_ids"][0, st]  # every start labelled: its gradient is zero because it is a start
    return b


@functools.lru_cache(maxsize=None)
def nonfinite_base():
    return build_packed([40, 60, 80, 50, 70], 209, C=0.1, overflow_share=0.0)


def nonfinite_subcases():
    """name -> (loss config, column edits {name: value} applied to ONE token)."""
    ent_off = dict(NF_CFG, entropy_bonus=0.0, final_entropy_bonus=0.0)
    return {
        "nan_advantage": (NF_CFG, dict(advantages=np.nan)),
        "inf_advantage": (NF_CFG, dict(advantages=np.inf)),
        "nan_reward": (NF_CFG, dict(rewards=np.nan)),                                          # a statistic only: max / min report it
        "ratio_inf_positive_advantage": (NF_CFG, dict(delta_new_old=90.0, advantages=0.7)),   # the clipped side keeps the token finite
        "ratio_inf_negative_advantage": (NF_CFG, dict(delta_new_old=90.0, advantages=-0.7)),  # min() takes -inf
        "ratio_squared_overflows": (NF_CFG, dict(delta_new_old=50.0, advantages=-0.7)),       # ratio 5e21 finite, its square is not
        "nan_entropy_with_the_term": (NF_CFG, dict(entropy=np.nan)),
        "nan_entropy_without_the_term": (ent_off, dict(entropy=np.nan)),
        "num_labels_zero": (NF_CFG, dict(num_labels=0.0)),
        "num_labels_half": (NF_CFG, dict(num_labels=0.5)),
        "nan_new_logprob": (NF_CFG, dict(new_logprobs=np.nan)),                                # the three counters
    }


def poisoned(name, labelled=True):
    """(loss config, batch with the sub-case's edit on one token, index of that token)."""
    cfg, edit = nonfinite_subcases()[name]
    b = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in nonfinite_base().items()}
    lab = b["labels"][0] != -100
    want = np.flatnonzero((lab == labelled) & (np.arange(lab.size) > 100) & (b["position_ids"][0] > 0))
    u = int(want[7])
    for k, v in edit.items():
        if k == "delta_new_old":
            b["old_logprobs"][0, u] = b["new_logprobs"][0, u] - F32(v)
        else:
            b[k][0, u] = v
    return cfg, b, u


@functools.lru_cache(maxsize=1)
def e2e_logits():
    g = torch.Generator().manual_seed(210)
    return (torch.randn(1, E2E_T, E2E_V, generator=g) * 2).numpy()


def e2e_batch(new, entropy):
    """The `branches` table on log-probs / entropies of a model ([T], token-aligned); ref - new at +-C / 2, +-3C / 4, +-2C.  +-C itself
    is not reachable exactly from a given log-prob, and neither is 0 in the fused kernel, which forms its own log-probs, an ulp or two
    from the forward kernel's: at ref - new = 0 that ulp is the whole KL gradient (kl_coef * w * 9.5e-7 at a log-prob of -11), and on a
    token whose policy term is 0 it showed as 1.7e-2 of the entropy-only d logits scale - the |cl| -> 0 region build_packed keeps out of
    for want of a yardstick.  Exactly 0 is the `branches` case's, on given log-probs; here its cell holds +-3C / 4, where an ulp of a
    log-prob of -11 is 1.8e-6 of the KL gradient."""
    b = build_packed(_e2e_lens(), 212, table=True, C=1.0, new=new, entropy=entropy, overflow_share=0.0)
    t = b["ref_logprobs"].astype(np.float64) - b["new_logprobs"]
    inside = np.where(np.arange(t.shape[1]) % 2 == 0, 0.75, -0.75)
    target = np.select([np.abs(np.abs(t) - 1.0) < 0.1, t == 0.0], [0.5 * np.sign(t), inside], t)
    b["ref_logprobs"] = (b["new_logprobs"].astype(np.float64) + target).astype(F32)
    return b


def _e2e_lens():
    rng = np.random.default_rng(213)
    lens, left = [], E2E_T
    while left > 0:
        n = int(min(left, rng.integers(20, 120)))
        lens.append(n)
        left -= n
    return lens


def e2e_ids():
    return build_packed(_e2e_lens(), 212, table=True, C=1.0)["input_ids"]  # the ids depend on the seed only


def e2e_host_batch():
    """The e2e case with fp64 log-probs / entropies rounded to fp32 in place of the forward kernel's (for the CPU measurement)."""
    logits, ids = e2e_logits(), e2e_ids()
    nlp, ent, _ = gc.forward_witness(logits[0, :-1], ids[0, 1:], 1.0)
    return e2e_batch(np.concatenate([[0.0], nlp]), np.concatenate([[0.0], ent]))


def cut_batch(b, cut):
    return {k: (np.ascontiguousarray(v[:, :cut]) if isinstance(v, np.ndarray) else v) for k, v in b.items()}


def host_cases(name):
    """(label, loss config, batch, flat) of every launch configuration of a case: what the oracle is measured on."""
    if name == "branches":
        return [(cfg_id(c), c, branches_batch(), False) for c in BRANCH_CFGS]
    if name == "tie":
        return [(cfg_id(c), c, tie_batch(), False) for c in TIE_CFGS]
    if name == "nonfinite":
        out = [("base", NF_CFG, nonfinite_base(), False)]
        for n in nonfinite_subcases():
            for labelled in (True, False):
                c, b, _ = poisoned(n, labelled)
                out.append((f"{n} labelled={labelled}", c, b, False))
        return out
    if name == "rounds":
        return [(f"flat={f}", ROUNDS_CFG, rounds_batch(), f) for f in (False, True)]
    if name == "padded":
        return [(f"B={B} L={L} {side}", PADDED_CFG, padded_batch(B, L, side), False) for B, L, side in PADDED_SHAPES]
    if name == "flat":
        return [(f"flat={f}", FLAT_CFG, flat_batch(), f) for f in (True, False)]
    if name == "e2e":
        return [("host log-probs", E2E_CFG, e2e_host_batch(), False)]
    raise KeyError(name)


CASE_NAMES = ("branches", "tie", "nonfinite", "rounds", "padded", "flat", "e2e")


@functools.lru_cache(maxsize=8)
def _rounds_witness(flat):
    return tc.witness(ROUNDS_CFG, **tc.columns(rounds_batch()), flat=flat)


# ---- device side -------------------------------------------------------------------------------------------------------------
FLOAT_COLS = ("new_logprobs", "entropy", "old_logprobs", "ref_logprobs", "advantages", "rewards", "group_tokens", "num_labels", "overflow")


def c_cfg_of(cfg, flat=False):
    from pipelinerl_amd.finetune.rl import RLConfig, make_loss_config

    c = make_loss_config(RLConfig(**cfg), 0, 10)[0]
    c.flat_micro_batches = 1 if flat else 0
    return c


def upload(batch, dev, misalign=False):
    """The kernel's input columns on the device; `misalign`: every column 4 bytes (fp32) / 8 bytes (int64) off 16-byte alignment."""
    def put(a, dtype):
        t = torch.from_numpy(np.ascontiguousarray(a)).to(dev).to(dtype)
        if misalign:
            buf = torch.empty(t.numel() + 1, dtype=dtype, device=dev)
            buf[1:] = t.reshape(-1)
            return buf[1:].view_as(t)
        return t
    d = {k: put(batch[k], torch.float32) for k in FLOAT_COLS}
    d["labels"] = put(batch["labels"], torch.long)
    d["position_ids"] = put(batch["position_ids"], torch.long) if batch.get("is_packed") and batch["labels"].shape[0] == 1 else None
    assert (d["labels"].data_ptr() % 16 != 0) == misalign or d["labels"].numel() == 0
    return d


def launch(lib, d, c_cfg, want_grad=True):
    """`prl_grpo_loss_fwd_bwd` as `grpo_loss_from_logprobs` issues it, into NaN-filled outputs -> (loss, stats dict, g_nlp, g_ent) numpy."""
    from pipelinerl_amd import _lib
    from pipelinerl_amd._lib import STAT_INDEX
    from pipelinerl_amd.finetune.rl import _loss_workspace

    dev = d["labels"].device
    rows, cols = d["labels"].shape
    nan = float("nan")
    stats = torch.full((_lib.PRL_NUM_STATS,), nan, dtype=torch.float64, device=dev)
    loss = torch.full((), nan, dtype=torch.float32, device=dev)
    g_nlp = torch.full((rows, cols), nan, dtype=torch.float32, device=dev) if want_grad else None
    g_ent = torch.full((rows, cols), nan, dtype=torch.float32, device=dev) if (want_grad and c_cfg.use_entropy_loss) else None
    ws = _loss_workspace(dev)
    p = _lib.ptr
    with torch.cuda.device(dev):
        _lib.check(lib.prl_grpo_loss_fwd_bwd(
            ctypes.byref(c_cfg), rows, cols, p(d["labels"]), p(d["position_ids"]), p(d["new_logprobs"]), p(d["entropy"]), p(d["old_logprobs"]),
            p(d["ref_logprobs"]), p(d["advantages"]), p(d["rewards"]), p(d["group_tokens"]), p(d["num_labels"]), p(d["overflow"]), None, None,
            p(g_nlp), p(g_ent), p(loss), p(stats), p(ws), ws.numel(), _lib.current_stream_ptr(dev)))
    torch.cuda.synchronize()
    s = stats.cpu().numpy()
    sd = {k: float(s[i]) for k, i in STAT_INDEX.items()}
    assert float(np.float32(sd["loss"])) == loss.item() or (np.isnan(sd["loss"]) and np.isnan(loss.item()))
    return loss.item(), sd, (g_nlp.cpu().numpy() if g_nlp is not None else None), (g_ent.cpu().numpy() if g_ent is not None else None)


def held(label, got, w, grads=True):
    """Print the measured metrics next to their bounds and assert them: (loss, stats, g_nlp, g_ent) of `launch` against a witness."""
    _, sd, g_nlp, g_ent = got
    rs = tc.check_stats(sd, w)
    line = f"[token] {label}: statistics {rs.err:.3e} ({rs.name}; bound {tc.STAT_BOUND:.1e}); loss {rs.loss_err:.3e} (bound {tc.LOSS_BOUND:.1e}); max / min kl {rs.kl_err:.3e}"
    if grads:
        rt = tc.check_tokens(g_nlp, g_ent, w)
        line += f"; g_nlp per token {rt.err:.3e}, g_ent {rt.ent_err:.3e} (bound {tc.TOKEN_BOUND:.1e}); {rt.stray} stray"
    print(line)
    assert rs.ok(), f"{label}: {rs}"
    if grads:
        assert rt.ok(), f"{label}: {rt}"
        return rs, rt
    return rs, None


def same_bits(label, a, b):
    n, at = tc.n_bit_differences(a, b)
    assert n == 0, f"{label}: {n} entries differ bit for bit, first at {at}"


@pytest.mark.parametrize("policy", ["ppo", "reinforce"])
def test_branches(libprl, cuda_device, policy):
    b = branches_batch()
    d = upload(b, cuda_device)
    for cfg in (c for c in BRANCH_CFGS if c["policy_loss"] == policy):
        w = tc.witness(cfg, **tc.columns(b))
        held(f"branches {cfg_id(cfg)}", launch(libprl, d, c_cfg_of(cfg)), w)


def test_wrapper_is_the_same_launch(libprl, cuda_device):
    from pipelinerl_amd.finetune.rl import grpo_loss_from_logprobs
    from pipelinerl_amd.finetune.types import PipelineBatchEncoding

    b = branches_batch()
    d = upload(b, cuda_device)
    cfg = BRANCH_CFGS[-1]
    fields = {k: torch.from_numpy(v).to(cuda_device) if isinstance(v, np.ndarray) else v for k, v in b.items() if k not in ("new_logprobs", "entropy")}
    pb = PipelineBatchEncoding(**fields)
    loss, stats, g_nlp, g_ent = grpo_loss_from_logprobs(c_cfg_of(cfg), pb, d["new_logprobs"], d["entropy"])
    got = launch(libprl, d, c_cfg_of(cfg))
    assert loss.item() == got[0]
    same_bits("wrapper g_nlp", g_nlp.cpu().numpy(), got[2])
    same_bits("wrapper g_ent", g_ent.cpu().numpy(), got[3])
    assert np.array_equal(stats.cpu().numpy(), np.asarray(list(got[1].values())), equal_nan=True)


def test_exact_tie(libprl, cuda_device):
    """epsilon = 0 and new == old: ratio = 1 = clip_lo = clip_hi.  The clamp changes nothing (indicator 0), min() ties and splits the
    gradient over two equal halves, the inclusive inside rule keeps both: the full gradient."""
    b = tie_batch()
    d = upload(b, cuda_device)
    for cfg in TIE_CFGS:
        w = tc.witness(cfg, **tc.columns(b))
        assert (w.ratio[w.mask] == 1.0).all() and w.stats["clamp_log_ratio_new_old_indicator"] == 0
        got = launch(libprl, d, c_cfg_of(cfg))
        held(f"tie {cfg_id(cfg)}", got, w)
        assert got[1]["clamp_log_ratio_new_old_indicator"] == 0


def _class(x):
    x = float(np.float32(x))
    if np.isnan(x):
        return "nan"
    if np.isinf(x) or abs(x) >= tc.FLT_MAX:
        return ("+" if x > 0 else "-") + ("inf" if np.isinf(x) else "max")
    return "finite"


@pytest.mark.parametrize("name", list(nonfinite_subcases()))
def test_nonfinite(libprl, cuda_device, name):
    """One poisoned token among ordinary ones.  Its own gradients follow the witness (exactly 0 when loss_t w is not finite); every other
    token's are bit-equal to the same launch with that token unlabelled; the counters are exact; every public statistic, after the
    fp32 cast of `stats_to_dict`, is in the same class as the oracle's fp32 value (NaN, +-inf, +-FLT_MAX or finite) and the finite
    ones are held to the witness under STAT_BOUND, as the oracle's are on the CPU.  On an unlabelled token the same poison changes
    nothing but the three counters."""
    from pipelinerl_amd.finetune.rl import stats_to_dict

    base = launch(libprl, upload(nonfinite_base(), cuda_device), c_cfg_of(nonfinite_subcases()[name][0]))
    for labelled in (True, False):
        cfg, b, u = poisoned(name, labelled)
        w = tc.witness(cfg, **tc.columns(b))
        got = launch(libprl, upload(b, cuda_device), c_cfg_of(cfg))
        held(f"nonfinite {name} labelled={labelled}", got, w)
        if labelled:
            if not w.finite[u]:
                assert got[2][0, u] == 0 and (got[3] is None or got[3][0, u] == 0)
            b2 = dict(b, labels=b["labels"].copy())
            b2["labels"][0, u] = -100
            other = launch(libprl, upload(b2, cuda_device), c_cfg_of(cfg))
            keep = np.arange(b["labels"].size) != u
            same_bits(f"{name}: g_nlp of the other tokens", got[2][0, keep], other[2][0, keep])
            if got[3] is not None:
                same_bits(f"{name}: g_ent of the other tokens", got[3][0, keep], other[3][0, keep])
        else:
            same_bits(f"{name} unlabelled: g_nlp", got[2], base[2])
            if got[3] is not None:
                same_bits(f"{name} unlabelled: g_ent", got[3], base[3])
            assert got[0] == base[0]
            for k, v in got[1].items():
                if not k.startswith("nonfinite"):
                    assert v == base[1][k], (name, k, v, base[1][k])
        for k in ("nonfinite_new_logprobs", "nonfinite_log_ratio_ref_new", "nonfinite_kl", "bad_group_tokens"):
            assert got[1][k] == w.stats[k] == (1.0 if (name == "nan_new_logprob" and not k.startswith("bad")) else 0.0), (name, k)
        _, _, ostats = tc.oracle_fp32(cfg, b)
        s = [got[1][k] for k in got[1]]
        public = stats_to_dict(s, 0.05, 0.01, b["labels"].size)
        for k, ov in ostats.items():
            if k in public and k != "num_output_tokens_sum":
                assert _class(public[k]) == _class(ov), (name, labelled, k, public[k], ov)


def test_paths(libprl, cuda_device):
    """The `branches` table three ways - aligned with gradients (4 tokens per lane, FAST), aligned without (2 per lane, FAST;
    statistics and loss only), 4 / 8 bytes off alignment (1 per lane, the branchy fallback) - at T, T - 1, T - 2, T - 3.  All are
    held to the witness; the gradients of the aligned and the misaligned launch are bit-equal (the same instruction sequence)."""
    full = branches_batch()
    T = full["labels"].shape[1]
    for cut in (T, T - 1, T - 2, T - 3):
        b = cut_batch(full, cut)
        da, dm = upload(b, cuda_device), upload(b, cuda_device, misalign=True)
        for cfg in BRANCH_CFGS[::3] + [BRANCH_CFGS[-1]]:
            w = tc.witness(cfg, **tc.columns(b))
            label = f"paths cut {cut} {cfg_id(cfg)}"
            ga = launch(libprl, da, c_cfg_of(cfg))
            held(label + " aligned", ga, w)
            held(label + " no gradient", launch(libprl, da, c_cfg_of(cfg), want_grad=False), w, grads=False)
            gm = launch(libprl, dm, c_cfg_of(cfg))
            held(label + " misaligned", gm, w)
            same_bits(label + ": g_nlp aligned vs misaligned", ga[2], gm[2])
            if ga[3] is not None:
                same_bits(label + ": g_ent aligned vs misaligned", ga[3], gm[3])


_ROUNDS_DEV = {}


def _rounds_dev(dev, misalign=False):
    if misalign not in _ROUNDS_DEV:
        _ROUNDS_DEV[misalign] = upload(rounds_batch(), dev, misalign)
    return _ROUNDS_DEV[misalign]


@pytest.mark.parametrize("flat", [False, True], ids=["packed", "flat_micro_batches"])
def test_rounds(libprl, cuda_device, flat):
    """One launch of 4 199 427 tokens: more than two rounds of the largest possible grid (2048 blocks x 256 lanes) at 4, 2 and 1
    tokens per lane, whatever the occupancy query returns; the last round is ragged and 3 tokens are left to the scalar tail.
    Every g_nlp[u] and g_ent[u] is checked."""
    b = rounds_batch()
    assert b["labels"].shape[1] == ROUNDS_T > 2 * 2048 * 256 * 4 and ROUNDS_T % 4 == 3
    w = _rounds_witness(flat)
    assert w.mask.sum() > 2_500_000
    d = _rounds_dev(cuda_device)
    held(f"rounds flat={flat}", launch(libprl, d, c_cfg_of(ROUNDS_CFG, flat)), w)
    held(f"rounds flat={flat} no gradient", launch(libprl, d, c_cfg_of(ROUNDS_CFG, flat), want_grad=False), w, grads=False)
    if not flat:
        dm = upload(b, cuda_device, misalign=True)
        held("rounds misaligned", launch(libprl, dm, c_cfg_of(ROUNDS_CFG, flat)), w)


def test_rounds_are_reproducible(libprl, cuda_device):
    d = _rounds_dev(cuda_device)
    runs = [launch(libprl, d, c_cfg_of(ROUNDS_CFG, True)) for _ in range(4)]
    for r in runs[1:]:
        assert r[0] == runs[0][0]
        assert np.array_equal(np.asarray(list(r[1].values())).view(np.uint64), np.asarray(list(runs[0][1].values())).view(np.uint64))
        same_bits("g_nlp", r[2], runs[0][2])
        same_bits("g_ent", r[3], runs[0][3])
    _ROUNDS_DEV.clear()


@pytest.mark.parametrize("L", [1, 2, 3, 5, 7, 1023, 1025])
def test_padded(libprl, cuda_device, L):
    for B, side in itertools.product((1, 2, 3, 257), ("right", "left")):
        b = padded_batch(B, L, side)
        d = upload(b, cuda_device)
        w = tc.witness(PADDED_CFG, **tc.columns(b))
        got = launch(libprl, d, c_cfg_of(PADDED_CFG))
        held(f"padded B={B} L={L} {side}", got, w)
        assert got[1]["num_sequences"] == B and got[1]["bad_group_tokens"] == 0
        assert not got[2][:, 0].any() and not got[3][:, 0].any()
        if L == 1:
            assert got[1]["num_output_tokens_sum"] == 0 and got[0] == 0 and not got[2].any() and not got[3].any()
        # group normalization: the reference's `group_tokens > 0` assert looks at padding too - exactly those positions are counted
        gn = dict(PADDED_CFG, group_normalization=True)
        wg = tc.witness(gn, **tc.columns(b))
        gg = launch(libprl, d, c_cfg_of(gn))
        pad = (b["group_tokens"][:, 1:] <= 0).sum()
        assert gg[1]["bad_group_tokens"] == wg.stats["bad_group_tokens"] == pad
        rt = tc.check_tokens(gg[2], gg[3], wg)
        assert rt.ok(), f"padded B={B} L={L} {side} group normalization: {rt}"


def test_flat_starts(libprl, cuda_device):
    b = flat_batch()
    st = flat_starts()
    d = upload(b, cuda_device)
    for flat in (True, False):
        w = tc.witness(FLAT_CFG, **tc.columns(b), flat=flat)
        got = launch(libprl, d, c_cfg_of(FLAT_CFG, flat))
        held(f"flat starts flat={flat}", got, w)
        assert got[1]["num_sequences"] == len(st)
        if flat:
            assert not got[2][0, st].any() and not got[3][0, st].any()
        else:
            assert np.count_nonzero(got[3][0, st[1:]]) == len(st) - 1 and got[2][0, 0] == 0
        assert got[1]["num_output_tokens_sum"] == w.mask.sum()


class FakeModel(torch.nn.Module):
    def __init__(self, logits):
        super().__init__()
        self.logits = torch.nn.Parameter(logits)

    def forward(self, **kwargs):
        return types.SimpleNamespace(logits=self.logits)


def test_end_to_end(libprl, cuda_device):
    """The `branches` ratios placed through the kernels' own forward (V = 1031): token gradients of the two-pass path against the
    witness, d logits of both modes per entry with the witness's token gradients."""
    from pipelinerl_amd.finetune.rl import RLConfig, logprob_entropy, rl_step
    from pipelinerl_amd.finetune.types import PipelineBatchEncoding

    logits = e2e_logits()
    ids = e2e_ids()
    lg = torch.from_numpy(logits).to(cuda_device)
    nlp, ent, _, _ = logprob_entropy(lg, torch.from_numpy(ids).to(cuda_device), 1.0)
    b = e2e_batch(nlp.cpu().numpy()[0], ent.cpu().numpy()[0])
    assert np.array_equal(b["input_ids"], ids)
    w = tc.witness(E2E_CFG, **tc.columns(b))
    assert {0.90, 1.10} <= set(np.round(w.ratio[w.mask], 2)) and w.stats["clamp_log_ratio_ref_new_indicator"] > 0
    held("e2e two-pass token gradients", launch(libprl, upload(b, cuda_device), c_cfg_of(E2E_CFG)), w)
    fields = {k: torch.from_numpy(v).to(cuda_device) if isinstance(v, np.ndarray) else v for k, v in b.items() if k not in ("new_logprobs", "entropy")}
    pb = PipelineBatchEncoding(**fields)
    rid, g, gh = gc.token_rows(b["input_ids"], w.g_nlp[None, 1:], w.g_ent[None, 1:])
    # a case built as meant has rows of both kinds: the policy term is non-zero on 8 of the table's 20 ratio x advantage cells and the
    # KL term on 3 of its 5 `ref - new` cells (0.76 of the labelled tokens together), the rest are labelled rows of zero gradient
    labelled = int(w.mask.sum())
    assert np.count_nonzero(g) == np.count_nonzero(w.g_nlp) and labelled // 2 < np.count_nonzero(g) < labelled
    for mode, fused in (("two_pass", False), ("fused", True)):
        model = FakeModel(lg.clone())
        loss, stats = rl_step(model, pb, 0, 10, RLConfig(**E2E_CFG, fused_logits_grad=fused))
        loss.backward()
        err = abs(loss.item() - w.loss) / w.loss_scale
        res = gc.dlogits_error(model.logits.grad.cpu().numpy()[0], logits[0], rid, g, gh, 1.0)
        print(f"[token] e2e {mode}: loss {err:.3e} (bound {tc.LOSS_BOUND:.1e}); [dlogits] per entry {res.err:.3e} (bound {gc.DLOGITS_BOUND['k1_random_g']:.1e})")
        # the fused kernel forms its own log-probs (ulps from the forward kernel's, which the witness was built on): its loss is printed only
        assert (err <= tc.LOSS_BOUND or fused) and stats["loss"] == loss.item()
        assert res.ok(gc.DLOGITS_BOUND["k1_random_g"]), str(res)
