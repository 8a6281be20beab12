"""The per-segment check of the sequence-level (GSPO) term (tests/seq_term_checks.py) tested on the CPU: the witness reproduces
the reference's goldens, the oracle's own fp32 arithmetic stays within the values the bounds were derived from on every case the
GPU tests run (`test_gpu_gspo_edges.case`), every mutant of a correct result is rejected, and a badly built case is refused.

The mutants are numpy edits of a correct result that imitate what a subtly wrong kernel writes: nothing here runs a kernel."""

import numpy as np
import pytest

from oracle import rl_loss as orl

import grad_checks as gc
import seq_term_checks as sc
import test_gpu_gspo_edges as ge
from helpers import load_rl_case, rel_err

FP_TOL = 1e-4
F32 = np.float32


def test_config_scalars_are_the_loss_configs():
    """clip_lo / clip_hi / the batch weight of the witness are the fp32 values `make_loss_config` hands the kernels."""
    from pipelinerl_amd.finetune.rl import RLConfig, make_loss_config

    for cfg in ge.ALL_CFGS + [ge.loss_cfg(eps=0.0), ge.loss_cfg(eps=0.002), ge.loss_cfg(eps=0.004)]:
        c, _, _ = make_loss_config(RLConfig(**cfg), 0, 10)
        assert (float(c.clip_lo), float(c.clip_hi)) == sc.clip_bounds(cfg)
        if not cfg["group_normalization"]:
            assert float(c.token_weight) == float(F32(1) / F32(cfg["batch_size"]))
    assert sc.COEF_BOUND < gc.MUTANT_FLOOR and sc.COEF_BOUND > 0 and sc.LOSS_BOUND > 0
    assert set(sc.SEQ_REF) == set(ge.CASE_NAMES)


@pytest.mark.parametrize("name", ["c11_gspo", "c12_gspo_groupnorm_sp", "c21_gspo_value_head"])
def test_witness_reproduces_the_goldens(name):
    case = load_rl_case(name)
    cfg, b = case["config"], case["batch"]
    nlp, ent, p, _ = orl.logprob_entropy(case["logits"], b["input_ids"], cfg.get("temperature", 1.0))
    ref = orl.token_loss(b, nlp, ent, cfg, *case["steps"], True, value=case.get("value"))
    want_loss = case["loss"]
    if "value" in case:  # value head: the advantages column is rewards - V, the value loss is a separate kernel's
        b = dict(b, advantages=np.concatenate([np.zeros_like(b["rewards"][:, :1]), b["rewards"][:, 1:] - case["value"][:, :-1]], axis=1))
        want_loss = case["loss"] - cfg["value_loss_coef"] * case["stats"]["value_loss"]
    new = np.concatenate([np.zeros((1, 1), dtype=F32), nlp], axis=1)
    w = sc.witness(cfg, b["segment_ids"], b["labels"], new, b["old_logprobs"], b["advantages"], b["group_tokens"], b["overflow"])
    print(f"{name}: loss {w.loss:.9e} (golden {want_loss:.9e}), {len(w.coef)} segments, {int(w.indicator.sum())} clipped")
    assert abs(w.loss - want_loss) <= 1e-5 * max(abs(want_loss), 1e-6)
    mask = (b["labels"] != -100)[0, 1:]
    g = w.ext_g[1:] * mask
    np.testing.assert_allclose(g, ref["g_nlp"][0], rtol=1e-5, atol=0)
    # and the golden's own autograd: d logits = g (1[v = id] - p_v) / temperature (GSPO has no other token gradient)
    T, V = p.shape[1] + 1, p.shape[2]
    onehot = np.zeros((T - 1, V))
    onehot[np.arange(T - 1), b["input_ids"][0, 1:]] = 1.0
    grad = np.zeros((T, V))
    grad[:-1] = g[:, None] * (onehot - p[0]) / cfg.get("temperature", 1.0)
    if np.abs(case["grad_logits"]).max() > 0:
        assert rel_err(grad, case["grad_logits"][0]) <= FP_TOL
    clamp = float((w.ext_c[1:][mask] / b["num_labels"][0, 1:][mask]).sum())
    assert abs(clamp - case["stats"]["clamp_log_ratio_new_old_indicator"]) <= 2e-5


def _oracle_check(name, batch, cfg, extra):
    """(TermsCheck of the oracle's fp32 branch against the witness, the witness) on one case and loss config."""
    gs = extra.get("grad_scale", 1.0)
    if name == "slice":  # the oracle sees the whole sequence; the slice's witness takes the whole sequence's sums
        whole = sc.witness(cfg, *ge.columns(extra["whole"]))
        w = sc.witness(cfg, *ge.columns(batch), n_segments=ge.SLICE_SEGMENTS, sums=whole.sums, grad_scale=gs)
        coef, loss, res = ge.oracle_terms(extra["whole"], cfg, gs)
        stat_w, stat_b = whole, extra["whole"]
    else:
        w = sc.witness(cfg, *ge.columns(batch))
        coef, loss, res = ge.oracle_terms(batch, cfg, gs)
        stat_w, stat_b = w, batch
    if len(coef) < len(w.coef):  # the oracle sizes by the largest id on the shifted axis
        coef = np.concatenate([coef, np.zeros(len(w.coef) - len(coef))])
    rt = sc.check_terms(coef, w.indicator, loss, w)  # the oracle does not expose its per-segment indicator: its statistic below
    lab = stat_b["labels"][0] != -100
    lab[0] = False
    clamp = float((stat_w.ext_c[lab] / stat_b["num_labels"][0][lab]).sum())
    assert abs(res["stats"]["clamp_log_ratio_new_old_indicator"] - clamp) <= FP_TOL * max(clamp, 1.0)
    return rt, w


@pytest.mark.parametrize("name", ge.CASE_NAMES)
def test_oracle_fp32_stays_within_the_written_values(name):
    """The yardstick of COEF_BOUND / LOSS_BOUND: the oracle's fp32 GSPO branch on every GPU case, measured again."""
    batch, cfgs, extra = ge.case(name)
    ref_coef, ref_loss = sc.SEQ_REF[name]
    worst = [0.0, 0.0]
    for cfg in cfgs:
        rt, w = _oracle_check(name, batch, cfg, extra)
        print(f"oracle fp32 {name} {ge._cfg_id(cfg)}: coef {rt.coef_err:.3e} at segment {rt.coef_seg} (written {ref_coef:.1e}, bound "
              f"{sc.COEF_BOUND:.1e}); loss {rt.loss_err:.3e} (written {ref_loss:.1e}, bound {sc.LOSS_BOUND:.1e})")
        assert rt.stray == 0, str(rt)
        assert rt.ok(), str(rt)
        worst = [max(worst[0], rt.coef_err), max(worst[1], rt.loss_err)]
    assert worst[0] <= ref_coef and worst[1] <= ref_loss, (name, worst)


def test_cases_are_what_the_issue_asks_for():
    g = ge.geometry_segments()
    lengths = [s["n"] for s in g]
    assert g[0]["n"] == 1 and {1, 2, 3, 255, 256, 257, 511, 512, 513, 8192} <= set(lengths) and sum(n <= 70 for n in lengths) >= 36
    assert {s["lab"] for s in g} >= {"none", "first", "last"} and any(s["ovf"] for s in g)
    assert len(ge.many_segments()) == 700 and all(1 <= s["n"] <= 5 for s in ge.many_segments())
    wide = ge.wide_segments()
    assert len(wide) == 300 and sum(s["n"] for s in wide) >= 1_200_000
    assert sum(s["n"] for s in ge.e2e_segments()) == ge.E2E_T
    b, _, _ = ge.case("slice")
    assert b["segment_ids"][0, 0] == ge.SLICE_FIRST and b["segment_ids"][0, -1] == ge.SLICE_SEGMENTS - 1
    for name in ge.CASE_NAMES:  # targets hit: every ratio is on a target of RATIOS (the truncated / NaN segments aside)
        batch, cfgs, extra = ge.case(name)
        if name in ("slice", "nan"):
            continue
        w = sc.witness(cfgs[0], *ge.columns(batch))
        live = w.sums[2] > 0
        assert np.isclose(w.ratio[live][:, None], np.asarray(ge.RATIOS)[None], rtol=1e-6, atol=0).any(axis=1).all(), name


def _correct(w):
    """A correct fp32 result: the witness rounded once."""
    return w.coef.astype(F32), w.indicator.astype(F32), F32(w.loss)


def test_mutants_of_the_sums_are_rejected():
    batch, cfgs, _ = ge.case("geometry")
    cfg = cfgs[3]
    w = sc.witness(cfg, *ge.columns(batch))
    assert sc.check_sums(w.sums.copy(), w).ok()
    mask, terms = sc.token_terms(cfg, *ge.columns(batch)[1:])
    seg = batch["segment_ids"][0]
    s = int(np.argmax(w.sums[2]))
    assert w.sums[2, s] == 8192
    run = np.flatnonzero((seg == s) & mask)

    def moved(u, to):
        m = w.sums.copy()
        m[:, s] -= terms[:, u]
        if to is not None:
            m[:, to] += terms[:, u]
        return m

    for label, m in (("one labelled token dropped from the longest segment", moved(run[4000], None)),
                     ("the first token of the run credited to the previous segment", moved(run[0], s - 1)),
                     ("the last token of the run credited to the next segment", moved(run[-1], s + 1))):
        rs = sc.check_sums(m, w)
        _, coef, _, _, _, _ = sc.segment_terms(cfg, m, guard=False)
        old = rel_err(sc.expand(seg, coef, w.indicator)[0][1:] * mask[1:], w.ext_g[1:] * mask[1:])
        own = abs(coef[s] - w.coef[s]) / abs(w.coef[s])
        print(f"mutant '{label}': {rs}; coef of the segment moves by {own:.2e}, max-norm of the token gradients {old:.2e}")
        assert not rs.ok(), label
        assert own < FP_TOL  # what no 1e-4 check on the 8192-token segment's own gradient can see
    # the same with the counts left alone (a token swapped for its neighbour's value): still rejected, by the derived bound alone
    m = w.sums.copy()
    m[0, s] += terms[0, run[0] - 1] - terms[0, run[0]]
    rs = sc.check_sums(m, w)
    assert rs.count_mismatch == 0 and not rs.ok()


def test_mutants_of_the_terms_are_rejected():
    batch, cfgs, _ = ge.case("geometry")
    cfg = cfgs[3]
    w = sc.witness(cfg, *ge.columns(batch))
    coef, ind, loss = _correct(w)
    ok = sc.check_terms(coef, ind, loss, w)
    print(f"a correct fp32 result: {ok}")
    assert ok.ok() and ok.coef_err <= 2.0 ** -24 and sc.check_tokens(*(a.astype(F32) for a in (w.ext_g, w.ext_c)), batch["segment_ids"], coef, ind)[0] == 0

    live = np.flatnonzero(w.coef != 0)
    s = int(live[np.argmin(np.abs(w.coef[live]))])
    m = coef.copy()
    m[s] *= F32(1.001)
    rt = sc.check_terms(m, ind, loss, w)
    old = rel_err(sc.expand(batch["segment_ids"], m, ind)[0], w.ext_g)
    print(f"mutant 'coef of segment {s} x 1.001': {rt.coef_err:.3e} (bound {sc.COEF_BOUND:.1e}); max-norm of the token gradients {old:.2e}")
    assert not rt.ok() and rt.coef_seg == s and old <= FP_TOL  # the max norm accepts it: that is the gap

    dead = np.flatnonzero(~w.valid)
    assert len(dead) >= 3
    for s in dead:
        m = coef.copy()
        m[s] = F32(1e-30)
        rt = sc.check_terms(m, ind, loss, w)
        assert rt.stray == 1 and rt.stray_seg == s and not rt.ok()
    m = ind.copy()
    m[dead[1]] = 1.0
    assert sc.check_terms(coef, m, loss, w).indicator_mismatch == 1
    assert not sc.check_terms(coef, ind, F32(w.loss + 4.1 * sc.LOSS_BOUND * w.loss_scale), w).ok()
    assert not sc.check_terms(coef, ind, np.nan, w).ok()
    m = coef.copy()
    m[live[0]] = np.nan
    assert not sc.check_terms(m, ind, loss, w).ok()


def test_strict_inside_rule_is_rejected_on_the_exact_tie():
    batch, cfgs, _ = ge.case("tie")
    for cfg in cfgs:
        w = sc.witness(cfg, *ge.columns(batch))
        assert sc.check_terms(*_correct(w), w).ok()
        _, strict, ind, _, loss, _ = sc.segment_terms(cfg, w.sums, strict_inside=True)
        live = w.coef != 0
        assert live.sum() >= 3 and np.array_equal(strict[live], 0.5 * w.coef[live])  # lo < ratio < hi halves the coefficient
        rt = sc.check_terms(strict.astype(F32), ind, loss, w)
        print(f"mutant 'strict inside rule on the exact tie' {ge._cfg_id(cfg)}: {rt}")
        assert not rt.ok() and abs(rt.coef_err - 0.5) < 1e-6
        # and a clamp that reports the bound itself as clipped
        assert sc.check_terms(*_correct(w)[:1], np.ones_like(w.indicator), w.loss, w).indicator_mismatch == len(w.indicator)


def test_slice_mutants_are_rejected():
    part, cfgs, extra = ge.case("slice")
    cfg = cfgs[0]
    whole = sc.witness(cfg, *ge.columns(extra["whole"]))
    w = sc.witness(cfg, *ge.columns(part), n_segments=ge.SLICE_SEGMENTS, sums=whole.sums, grad_scale=2.0)
    coef, ind, loss = _correct(w)
    seg = part["segment_ids"]
    g, c = sc.expand(seg, coef, ind)
    assert sc.check_terms(coef, ind, loss, w).ok() and sc.check_tokens(g, c, seg, coef, ind) == (0, None)
    # indicator indexed by the global id
    bad, at = sc.check_tokens(g, ind[seg[0]], seg, coef, ind)
    print(f"mutant 'indicator indexed by seg instead of seg - seg[0]': {bad} of {g.size} tokens differ, first at column {at}")
    assert bad > g.size // 2 and at == 0
    # coef indexed by the local id
    assert sc.check_tokens(coef[seg[0] - seg[0, 0]], c, seg, coef, ind)[0] > 0
    # grad_scale omitted
    w1 = sc.witness(cfg, *ge.columns(part), n_segments=ge.SLICE_SEGMENTS, sums=whole.sums, grad_scale=1.0)
    rt = sc.check_terms(w1.coef.astype(F32), ind, loss, w)
    print(f"mutant 'grad_scale omitted': {rt}")
    assert not rt.ok() and abs(rt.coef_err - 0.5) < 1e-6
    # zero_out ignored
    wz = sc.witness(cfg, *ge.columns(part), n_segments=ge.SLICE_SEGMENTS, sums=whole.sums, grad_scale=2.0, zero_out=True)
    assert wz.loss == 0 and not wz.coef.any() and np.array_equal(wz.indicator, w.indicator)
    rt = sc.check_terms(coef, ind, loss, wz)
    assert rt.stray == int((w.coef != 0).sum()) and not rt.ok()


def test_a_stale_token_past_the_capped_grid_is_rejected():
    batch, cfgs, _ = ge.case("wide")
    w = sc.witness(cfgs[0], *ge.columns(batch))
    coef, ind, _ = _correct(w)
    seg = batch["segment_ids"]
    g, c = sc.expand(seg, coef, ind)
    assert g.size > ge.EXPAND_GRID_COLUMNS and sc.check_tokens(g, c, seg, coef, ind) == (0, None)
    u = ge.EXPAND_GRID_COLUMNS + 5
    m = g.copy()
    m[u] = coef[seg[0, u] - 1]  # what an earlier launch left there
    assert m[u] != g[u]
    assert sc.check_tokens(m, c, seg, coef, ind) == (1, u)
    assert rel_err(m, g) <= 2.0  # one token of 1.2 million
    m = c.copy()
    m[-1] = 1.0 - m[-1]
    assert sc.check_tokens(g, m, seg, coef, ind) == (1, g.size - 1)
    m = g.copy()
    m[7] = -m[7] if m[7] == 0 else m[7]  # a zero of the other sign is not bit-equal
    if g[7] == 0:
        assert sc.check_tokens(m, c, seg, coef, ind) == (1, 7)


def test_guard_refuses_a_ratio_that_nearly_touches_a_bound():
    cfg = ge.loss_cfg()
    lo, hi = sc.clip_bounds(cfg)
    for near in (hi * (1 + 1e-6), hi * (1 - 1e-6), lo * (1 + 1e-6), lo * (1 - 5e-5)):
        b = ge.build([ge.seg(1), ge.seg(40, "all", 1.0, 1.0), ge.seg(64, "all", near, 1.0), ge.seg(9, "all", 1.10, -1.0)], 201)
        with pytest.raises(sc.BadCase, match="segment 2"):
            sc.witness(cfg, *ge.columns(b))
        assert sc.witness(cfg, *ge.columns(b), guard=False).ratio[2] == pytest.approx(near, rel=1e-7)
    # 2 % away: accepted; exactly on the bound (by construction): accepted
    sc.witness(cfg, *ge.columns(ge.build([ge.seg(1), ge.seg(64, "all", hi * 1.02, 1.0)], 202)))
    tie, cfgs, _ = ge.case("tie")
    w = sc.witness(cfgs[0], *ge.columns(tie))
    assert (w.ratio == w.lo).all() and (w.ratio == w.hi).all()
    # an id outside [0, n_segments) on a labelled token is refused too, not clamped silently
    with pytest.raises(sc.BadCase):
        sc.witness(cfg, *ge.columns(tie), n_segments=3)
