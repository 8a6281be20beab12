"""The per-token check of the token-level loss term (tests/token_term_checks.py) tested on the CPU: the DEVICE math
(`prl_token_eval` of csrc/prl_token_math.h, compiled with g++ -ffp-contract=off) follows the witness on every branch-edge case the
GPU tests run (`test_gpu_token_edges.host_cases`), the oracle's own fp32 arithmetic stays within the values the bounds were derived
from, every mutant of a correct result is rejected, and a badly built case is refused.

The mutants are numpy edits of a correct result that imitate what a subtly wrong kernel writes: nothing here runs a kernel."""

import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest

import grad_checks as gc
import seq_term_checks as sc
import test_gpu_token_edges as te
import token_term_checks as tc
from helpers import rel_err

ROOT = Path(__file__).resolve().parent.parent
F = ctypes.POINTER(ctypes.c_float)
F32 = np.float32
FIELDS = ("contrib", "g_nlp", "g_ent", "w", "A", "ratio_stat", "kl", "kl_new_old", "abs_lrno", "exp_lrrn", "exp_ref_old", "clamp_rn", "clamp_no",
          "bad_nlp", "bad_lrrn", "bad_kl")


@pytest.fixture(scope="module")
def tokmath(tmp_path_factory):
    from pipelinerl_amd._lib import PrlLossConfig

    out = tmp_path_factory.mktemp("harness") / "libtokmath.so"
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", f"-I{ROOT / 'include'}", "-o", str(out),
                           str(ROOT / "tests" / "harness" / "token_math_host.cpp")])
    lib = ctypes.CDLL(str(out))
    lib.prl_host_token_eval_all.restype = None
    lib.prl_host_token_eval_all.argtypes = [ctypes.POINTER(PrlLossConfig), ctypes.c_long] + [F] * 10
    return lib


def device_math(lib, cfg, batch, flat):
    """`prl_token_eval` on every token, then the selection `token_step` makes -> (stats dict, g_nlp [N], g_ent [N]); the sums in fp64."""
    w = tc.witness(cfg, **tc.columns(batch), flat=flat, guard=False)
    ins = [np.ascontiguousarray(batch[k], dtype=F32).reshape(-1) for k in te.FLOAT_COLS]
    n = ins[0].size
    out = np.zeros((16, n), dtype=F32)
    c_cfg = te.c_cfg_of(cfg, flat)
    lib.prl_host_token_eval_all(ctypes.byref(c_cfg), n, *[a.ctypes.data_as(F) for a in ins], out.ctypes.data_as(F))
    o = dict(zip(FIELDS, out))
    m, v = w.mask, w.valid
    nl = ins[7]
    nan0 = lambda x: np.nan_to_num(x.astype(F32), nan=0.0)  # noqa: E731 - fp32 nan_to_num: +-inf -> +-FLT_MAX
    with np.errstate(all="ignore"):
        per = lambda x: float(nan0((x / nl).astype(F32))[m].astype(np.float64).sum())  # noqa: E731
        rsq = (o["ratio_stat"] * o["ratio_stat"]).astype(F32)
        sums = [per(ins[5]), per(ins[1]), per(ins[2]), per(ins[0]), per(ins[3]), per(ins[4]), per(o["kl"]), per(o["kl_new_old"]), per(o["abs_lrno"]),
                per(o["ratio_stat"]), float(nan0(o["ratio_stat"])[m].astype(np.float64).sum()), float(nan0(rsq)[m].astype(np.float64).sum()),
                per(o["exp_lrrn"]), per(o["exp_ref_old"]), per(o["clamp_rn"]), per(o["clamp_no"]), per(o["w"])]
    stats = dict(zip(tc.SUM_STATS, sums))
    ext = lambda x, fn, e: float(fn(x[m])) if m.any() else e  # noqa: E731
    stats.update(loss=-float(o["contrib"][m].astype(np.float64).sum()), num_output_tokens_sum=float(m.sum()), num_sequences=w.stats["num_sequences"],
                 max_reward=ext(ins[5], np.max, -np.inf), min_reward=ext(ins[5], np.min, np.inf), max_advantage=ext(ins[4], np.max, -np.inf),
                 min_advantage=ext(ins[4], np.min, np.inf), max_token_weight=ext(o["w"], np.max, -np.inf), min_token_weight=ext(o["w"], np.min, np.inf),
                 max_kl=ext(o["kl"], np.max, -np.inf), min_kl=ext(o["kl"], np.min, np.inf),
                 nonfinite_new_logprobs=float(o["bad_nlp"][v].sum()), nonfinite_log_ratio_ref_new=float(o["bad_lrrn"][v].sum()),
                 nonfinite_kl=float(o["bad_kl"][v].sum()), bad_group_tokens=w.stats["bad_group_tokens"])
    return stats, np.where(m, o["g_nlp"], F32(0)), np.where(m, o["g_ent"], F32(0))


def test_config_scalars_are_the_loss_configs():
    """clip bounds, C, the coefficients and the batch weight of the witness are the fp32 values `make_loss_config` hands the kernels."""
    for cfg in te.BRANCH_CFGS + te.TIE_CFGS + [te.ROUNDS_CFG, te.PADDED_CFG, te.FLAT_CFG, te.NF_CFG, te.E2E_CFG]:
        c, s = te.c_cfg_of(cfg), tc.config_scalars(cfg)
        assert (float(c.clip_lo), float(c.clip_hi), float(c.clamp_log_ratio_ref_new), float(c.kl_coef), float(c.entropy_coef)) == \
            (s["lo"], s["hi"], s["C"], s["kl_coef"], s["ent_coef"])
        assert bool(c.use_entropy_loss) == s["use_entropy"]
        if not cfg["group_normalization"]:
            assert float(c.token_weight) == float(s["token_weight"])
    assert 0 < tc.TOKEN_BOUND < gc.MUTANT_FLOOR and tc.STAT_BOUND > 0 and tc.LOSS_BOUND > 0
    assert set(tc.TOKEN_REF) == set(te.CASE_NAMES) and tc.GUARD == sc.GUARD


def test_cases_are_what_the_issue_asks_for():
    b = te.branches_batch()
    w = tc.witness(te.BRANCH_CFGS[0], **tc.columns(b))
    m = w.mask
    r = np.round(w.ratio, 2)
    adv = b["advantages"][0]
    for target in te.RATIOS:  # every ratio x every advantage class (the sign bit tells 0.0 from -0.0), labelled
        for sel in (adv > 0, adv < 0, (adv == 0) & ~np.signbit(adv), (adv == 0) & np.signbit(adv)):
            assert (m & (r == target) & sel).sum() >= 5, (target, int((m & (r == target) & sel).sum()))
    assert np.isclose(w.ratio[m][:, None], np.asarray(te.RATIOS)[None], rtol=1e-6, atol=0).any(axis=1).all()
    for t in te.KL_TABLE:  # ref - new exactly on every target, +-C included
        assert (m & (w.lrrn == t)).sum() >= 50
    for ovf in (0.0, 1.0):
        assert (m & (b["overflow"][0] == ovf)).sum() >= 300
    assert (m & (b["rewards"][0] < 0)).any() and (m & (b["rewards"][0] > 0)).any()
    assert len(te.BRANCH_CFGS) == 64 and m.sum() > 1500
    rb = te.rounds_batch()
    assert rb["labels"].shape[1] == te.ROUNDS_T == 2 * 2048 * 256 * 4 + 5 * 1024 + 3
    lens = np.diff(np.flatnonzero(np.concatenate([rb["position_ids"][0] == 0, [True]])))
    assert lens.min() == 1 and lens.max() > 8000 and lens.max() <= 8192
    st = te.flat_starts()
    assert {int(s) % 4 for s in st if (s // 4) % 256 == 0 and s > 0} == {0, 1, 2, 3} and {int(s) % 4 for s in st if (s // 4) % 256 == 255} == {0, 1, 2, 3}
    assert st[0] == 0 and (te.flat_batch()["position_ids"][0, st] == 0).all() and (te.flat_batch()["position_ids"][0] == 0).sum() == len(st)
    assert len(te.PADDED_SHAPES) == 7 * 4 * 2
    p = te.padded_batch(3, 7, "right")
    assert p["labels"][1, 0] != -100 and (p["labels"][2] == -100).all() and (p["num_labels"][2] == 0).all() and (p["group_tokens"][2] == 0).all()


@pytest.mark.parametrize("name", [n for n in te.CASE_NAMES if n != "rounds"])
def test_device_math_follows_the_witness(tokmath, name):
    """csrc/prl_token_math.h on the CPU: per-token metric, exact zeros, counters, and the statistics summed in fp64 from its fields.
    `rounds` is left out: it reaches no branch of the header that the other cases do not, what it is about is the kernel's loop, and
    its 4.2 M tokens take 17 s here.  `device_math` takes the label mask, `num_sequences` and `bad_group_tokens` from the witness -
    they are the kernel's work, not the header's - so those three comparisons say nothing on the host; the GPU test makes them."""
    for label, cfg, batch, flat in te.host_cases(name):
        w = tc.witness(cfg, **tc.columns(batch), flat=flat)
        stats, g_nlp, g_ent = device_math(tokmath, cfg, batch, flat)
        rt, rs = tc.check_tokens(g_nlp, g_ent, w), tc.check_stats(stats, w)
        print(f"[token] device math on the host, {name} {label}: g_nlp {rt.err:.3e}, g_ent {rt.ent_err:.3e} (bound {tc.TOKEN_BOUND:.1e}); {rs}")
        assert rt.ok(), f"{name} {label}: {rt}"
        assert rs.ok(), f"{name} {label}: {rs}"
        assert not g_nlp[~w.finite & w.mask].any() and not g_ent[~w.finite & w.mask].any()


def _oracle_check(cfg, batch, flat):
    w = tc.witness(cfg, **tc.columns(batch), flat=flat)
    g, gh, stats = tc.oracle_fp32(cfg, batch, flat)
    return tc.check_tokens(g, gh, w), tc.check_stats(stats, w), w


@pytest.mark.parametrize("name", te.CASE_NAMES)
def test_oracle_fp32_stays_within_the_written_values(name):
    """The yardstick of TOKEN_BOUND / STAT_BOUND / LOSS_BOUND: the oracle's fp32 path on every GPU case, measured again."""
    ref = tc.TOKEN_REF[name]
    worst = [0.0, 0.0, 0.0]
    for label, cfg, batch, flat in te.host_cases(name):
        rt, rs, _ = _oracle_check(cfg, batch, flat)
        assert rt.stray == 0 and not rs.mismatch, f"{name} {label}: {rt}; {rs}"
        worst = [max(worst[0], rt.err, rt.ent_err, rs.kl_err), max(worst[1], rs.err), max(worst[2], rs.loss_err)]
    print(f"oracle fp32 {name}: token {worst[0]:.3e} (written {ref[0]:.1e}, bound {tc.TOKEN_BOUND:.1e}); statistics {worst[1]:.3e} (written "
          f"{ref[1]:.1e}, bound {tc.STAT_BOUND:.1e}); loss {worst[2]:.3e} (written {ref[2]:.1e}, bound {tc.LOSS_BOUND:.1e})")
    assert worst[0] <= ref[0] and worst[1] <= ref[1] and worst[2] <= ref[2], (name, worst)


def _correct(w):
    """A correct fp32 result: the witness rounded once."""
    return w.g_nlp.astype(F32), w.g_ent.astype(F32)


def _reject(label, rt_or_rs, bound, value):
    print(f"mutant '{label}': scores {value:.3e} against the bound {bound:.1e} (margin x {value / bound:.3g}); {rt_or_rs}")
    assert not rt_or_rs.ok(), label
    assert value > bound


def test_mutants_of_the_large_case_are_rejected():
    w = te._rounds_witness(False)
    g, gh = _correct(w)
    ok = tc.check_tokens(g, gh, w)
    assert ok.ok() and ok.err <= 2.0 ** -23
    live = np.flatnonzero(w.scale > 0)
    u = int(live[np.argmax(np.abs(w.g_nlp[live]) / w.scale[live])])  # a token whose terms do not cancel: the factor shows in full
    m = g.copy()
    m[u] *= F32(1.001)
    rt = tc.check_tokens(m, gh, w)
    _reject(f"g_nlp of token {u} of {g.size} x 1.001", rt, tc.TOKEN_BOUND, rt.err)
    print(f"  the max norm scores it {rel_err(m, w.g_nlp):.2e} against 1e-4")
    assert rt.at == u and rel_err(m, w.g_nlp) <= 1e-4  # the max norm accepts it: that is the gap
    # round two computed from round one's inputs: g[u] := g[u - round] past the first round of 2048 x 256 x 4 tokens
    rnd = 2048 * 256 * 4
    m = g.copy()
    m[rnd:] = g[:-rnd]
    rt = tc.check_tokens(m, gh, w)
    _reject("round two computed from round one's inputs", rt, tc.TOKEN_BOUND, max(rt.err, float(rt.stray)))
    # statistics
    stats = dict(w.stats)
    assert tc.check_stats(stats, w).ok()
    k = tc.SUM_STATS.index("kl")
    lab = np.flatnonzero(w.mask)
    stats["kl"] = w.stats["kl"] - float(w.terms[k][lab[::64]].sum())
    rs = tc.check_stats(stats, w)
    old = abs(stats["kl"] - w.stats["kl"]) / max(abs(w.stats["kl"]), 1.0)
    _reject("kl with every 64th labelled token dropped", rs, tc.STAT_BOUND, rs.err)
    print(f"  the suite's max(|want|, 1) form scores it {old:.2e} against 1e-4")
    assert rs.name == "kl"
    stats = dict(w.stats)
    nl = te.rounds_batch()["num_labels"][0].astype(np.float64)
    stats["kl"] = float((w.terms[k] * nl).sum())
    rs = tc.check_stats(stats, w)
    _reject("kl summed without / num_labels", rs, tc.STAT_BOUND, rs.err)


def test_mutants_of_the_branch_rules_are_rejected():
    b = te.branches_batch()
    base = te.loss_cfg(ent=True)
    for label, cfg, mutate in (("the clipped side given gradient (d2 = d1 outside the range)", base, "clipped_grad"),
                               ("the KL gradient kept outside +-C", base, "kl_outside"),
                               ("relu skipped on A < 0", te.loss_cfg(relu=True), "no_relu"),
                               ("overflow ignored", te.loss_cfg(of=True), "no_overflow")):
        w = tc.witness(cfg, **tc.columns(b))
        assert tc.check_tokens(*_correct(w), w).ok()
        wrong = tc.witness(cfg, **tc.columns(b), mutate=mutate)
        rt = tc.check_tokens(*_correct(wrong), w)
        _reject(label, rt, tc.TOKEN_BOUND, max(rt.err, rt.ent_err, float(rt.stray)))
        assert rt.stray > 0 or rt.err > 0.01
    t = te.tie_batch()
    for cfg in te.TIE_CFGS:
        w = tc.witness(cfg, **tc.columns(t))
        strict = tc.witness(cfg, **tc.columns(t), mutate="strict_inside")
        live = (w.scale > 0) & (t["advantages"][0] != 0)
        assert live.sum() > 100
        rt = tc.check_tokens(*_correct(strict), w)
        _reject("the strict inside rule on the exact tie", rt, tc.TOKEN_BOUND, rt.err)


def test_mutants_of_the_mask_are_rejected():
    # a gradient of 1e-30 on a non-finite token
    cfg, b, u = te.poisoned("ratio_inf_negative_advantage")
    w = tc.witness(cfg, **tc.columns(b))
    assert w.mask[u] and not w.finite[u] and w.g_nlp[u] == 0
    g, gh = _correct(w)
    g[u] = F32(1e-30)
    rt = tc.check_tokens(g, gh, w)
    assert rt.stray == 1 and rt.stray_at == u and not rt.ok()
    # column 0 of row 1 of a padded batch treated as valid
    p = te.padded_batch(3, 7, "right")
    w = tc.witness(te.PADDED_CFG, **tc.columns(p))
    one_row = {k: (v.reshape(1, -1) if isinstance(v, np.ndarray) else v) for k, v in p.items()}
    as_row = tc.witness(te.PADDED_CFG, **tc.columns(one_row))
    g, gh = _correct(w)
    assert as_row.g_nlp[7] != 0 and w.g_nlp[7] == 0
    g[7] = as_row.g_nlp[7]
    rt = tc.check_tokens(g, gh, w)
    assert rt.stray == 1 and rt.stray_at == 7 and not rt.ok()
    # a flat sequence start treated as valid
    f = te.flat_batch()
    w = tc.witness(te.FLAT_CFG, **tc.columns(f), flat=True)
    loose = tc.witness(te.FLAT_CFG, **tc.columns(f), flat=False)
    st = te.flat_starts()
    g, gh = _correct(w)
    assert not w.g_nlp[st].any() and np.count_nonzero(loose.g_ent[st]) == len(st) - 1
    g[st[3]], gh[st[3]] = loose.g_nlp[st[3]], loose.g_ent[st[3]]
    rt = tc.check_tokens(g, gh, w)
    assert rt.stray == 1 and rt.stray_at == st[3] and not rt.ok()
    stats = dict(w.stats, num_output_tokens_sum=w.stats["num_output_tokens_sum"] + 1)
    assert tc.check_stats(stats, w).mismatch == ["num_output_tokens_sum"]
    print(f"mutants 'gradient 1e-30 on a non-finite token', 'column 0 of row 1 valid', 'flat start valid': each one stray entry, bound 0")


def test_guard_refuses_a_case_that_nearly_touches_a_bound():
    b = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in te.branches_batch().items()}
    cfg = te.BRANCH_CFGS[0]
    lo, hi = sc.clip_bounds(cfg)
    u = int(np.flatnonzero(b["labels"][0] != -100)[40])
    for near in (hi * (1 + 1e-6), hi * (1 - 1e-6), lo * (1 + 1e-6), lo * (1 - 5e-5)):
        b["old_logprobs"][0, u] = F32(b["new_logprobs"][0, u] - np.log(near))
        with pytest.raises(tc.BadCase, match=f"token {u}"):
            tc.witness(cfg, **tc.columns(b))
        assert tc.witness(cfg, **tc.columns(b), guard=False).ratio[u] == pytest.approx(near, rel=1e-6)
    b["old_logprobs"][0, u] = F32(b["new_logprobs"][0, u] - np.log(hi * 1.02))
    tc.witness(cfg, **tc.columns(b))  # 2 % away: accepted
    b["ref_logprobs"][0, u] = F32(b["new_logprobs"][0, u] + 1.00001)
    with pytest.raises(tc.BadCase, match="ref - new"):
        tc.witness(cfg, **tc.columns(b))
    # on an unlabelled token nothing hangs on the decision: accepted
    b["ref_logprobs"][0, u] = b["new_logprobs"][0, u]
    v = int(np.flatnonzero(b["labels"][0] == -100)[5])
    b["old_logprobs"][0, v] = F32(b["new_logprobs"][0, v] - np.log(hi * (1 + 1e-6)))
    tc.witness(cfg, **tc.columns(b))
