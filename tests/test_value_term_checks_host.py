"""The per-entry check of the value-head branch (tests/value_term_checks.py) tested on the CPU: the witness reproduces the value
statistics and d loss / d value the reference itself produced (goldens c18-c23), the oracle's own fp32 arithmetic stays within the values
the bounds were derived from on every case the GPU tests run (`test_gpu_value_edges.host_cases`), every mutant of a correct result is
rejected, and a badly built case is refused.

The mutants are numpy edits of a correct result that imitate what a subtly wrong kernel writes: nothing here runs a kernel.  For each
one the test also evaluates the assertions the suite had before (`|got - want| <= 1e-4 max(1, |want|)` on the five statistics with max /
min equal - or, in `test_value_head_non_finite_and_unlabelled`, on value_loss / value_mse / value_mean only -, `rtol=1e-5, atol=1e-12` on
the gradient, zeros on unlabelled targets and the last column) ON THE SAME ARRAYS and states whether they accept it (`OLD_ACCEPTS`).
Where they reject it, the gap was one of reach: no test before had more than one row, more than 65 536 entries or sparse labels."""

import numpy as np
import pytest

import test_gpu_value_edges as ve
import value_term_checks as vc
from helpers import load_rl_case

F32 = np.float32
GOLDENS = ("c18_ppo_value_head", "c19_reinforce_value_head_unpacked", "c20_ppo_value_head_rewards_sp", "c21_gspo_value_head",
           "c22_ppo_value_head_groupnorm_overlong", "c23_sentinel_value_head")


def test_bounds_are_four_times_the_written_reference():
    assert set(vc.VALUE_REF) == set(ve.CASE_NAMES)
    for k, bound in enumerate((vc.VALUE_GRAD_BOUND, vc.VALUE_STAT_BOUND, vc.VALUE_LOSS_BOUND)):
        assert bound == 4.0 * max(v[k] for v in vc.VALUE_REF.values()) and 0 < bound < vc.MUTANT_FLOOR == 3e-4
    for cfg in (ve.value_cfg(), ve.value_cfg(False, True)):  # the batch weight of the witness is the fp32 value the kernels are handed
        assert float(ve.c_cfg_of(cfg).token_weight) == float(vc.token_weight(cfg))


@pytest.mark.parametrize("name", GOLDENS)
def test_witness_reproduces_the_reference_goldens(name):
    """The reference's own fp32 value statistics and autograd d loss / d value, packed (c18, c20-c23) and [B, L] (c19)."""
    case = load_rl_case(name)
    b, cfg = case["batch"], case["config"]
    w = vc.witness(cfg, value=case["value"], **vc.columns(b))
    coef = cfg["value_loss_coef"]
    rg = vc.check_grad(case["grad_value"].astype(np.float64) / coef, w)
    print(f"golden {name}: {rg}")
    assert rg.stray == 0 and rg.err <= vc.VALUE_GRAD_BOUND + 2.0 ** -24  # the reference's gradient carries the product with the coefficient
    if "sentinel" in name:
        assert not w.mask.any() and list(case["stats"]) == ["input_size"] and all(w.stats[k] == 0.0 for k in vc.VALUE_STAT_KEYS)
        return
    assert w.mask.any() and (b["labels"].shape[0] > 1) == ("unpacked" in name)
    rs = vc.check_stats({k: case["stats"][k] for k in vc.VALUE_STAT_KEYS}, w)
    print(f"golden {name}: {rs}")
    assert rs.ok(), rs


def test_cases_are_what_the_issue_asks_for():
    assert ve.SHAPES == [(1, 1), (1, 2), (1, 255), (1, 256), (1, 257), (7, 64), (3, 1001), (1, 262144), (1, 262145), (3, 87383)]
    assert 3 * 87383 == ve.ROUND + 5 and ve.ROUND == 262144
    for rows, cols in ve.PLACEMENT_SHAPES + [(3, 87383), (1, 262145)]:
        sparse = (rows, cols) in ve.PLACEMENT_SHAPES
        b, v = ve.build(rows, cols, seed=3, sparse=True) if sparse else ve.build(rows, cols)
        lab = b["labels"] != -100
        nl, ovf = b["num_labels"], b["overflow"]
        assert lab[:, 0].any(), "labels in column 0"
        seq = b["segment_ids"][0] if rows == 1 else np.repeat(np.arange(rows), cols)
        n_seq = int(seq.max()) + 1
        flat = lab.reshape(-1)
        per_seq = np.bincount(seq, weights=flat, minlength=n_seq)
        assert (per_seq == 0).sum() == 1 and n_seq >= 3, "one sequence without labels"
        assert len(set(seq[ovf.reshape(-1) == 1])) == 1 and flat[ovf.reshape(-1) == 1].any(), "one labelled sequence with overflow = 1"
        assert (np.diff(nl.reshape(-1)[np.r_[0, np.flatnonzero(np.diff(seq)) + 1]]) != 0).any(), "num_labels differs between neighbours"
        live = [r for r in range(rows) if per_seq[seq[r * cols + 1]] > 0]
        assert all(lab[r, 1] and lab[r, cols - 1] for r in live), "targets at column 1 and column cols - 1"
        starts = np.flatnonzero(np.diff(seq)) + 1
        both = [s for s in starts if flat[s - 1] and flat[s]]
        assert len(both) >= (rows - 3 if rows > 1 else n_seq - 3) and (len(both) >= 4 or (rows, cols) != (7, 64)), "labels on both sides of the row starts / segment boundaries"
        if sparse:
            assert flat.sum() <= 3 * (n_seq + rows) + 3
    for kind in ve.NONFINITE_KINDS:
        for labelled in (True, False):
            for shape in ve.NONFINITE_SHAPES:
                b, v, i = ve.poisoned(kind, labelled, shape)
                assert (b["labels"].reshape(-1)[i + 1] != -100) == labelled and (i + 1) % shape[1] != 0
                assert (b["group_tokens"].reshape(-1)[i + 1] == 0) == (kind == "group_tokens_zero") and np.isfinite(v.reshape(-1)[i]) == (kind in ("3e19", "group_tokens_zero"))


def _oracle_check(cfg, batch, value):
    w = vc.witness(cfg, value=value, **vc.columns(batch))
    adv, g, stats = vc.oracle_fp32(cfg, batch, value)
    return vc.check_advantages(adv, w), vc.check_grad(g, w), vc.check_stats(stats, w), w


@pytest.mark.parametrize("name", ve.CASE_NAMES)
def test_oracle_fp32_stays_within_the_written_values(name):
    """The yardstick of the three bounds: the oracle's fp32 path on every GPU case, measured again."""
    ref = vc.VALUE_REF[name]
    worst = [0.0, 0.0, 0.0]
    for label, cfg, batch, value in ve.host_cases(name):
        (n_adv, _), rg, rs, _ = _oracle_check(cfg, batch, value)
        assert n_adv == 0 and rg.stray == 0 and not rs.mismatch, f"{name} {label}: {rg}; {rs}"
        worst = [max(worst[0], rg.err), max(worst[1], rs.err), max(worst[2], rs.loss_err)]
    print(f"oracle fp32 {name}: d value {worst[0]:.3e} (written {ref[0]:.1e}, bound {vc.VALUE_GRAD_BOUND:.1e}); statistics {worst[1]:.3e} (written "
          f"{ref[1]:.1e}, bound {vc.VALUE_STAT_BOUND:.1e}); value_loss {worst[2]:.3e} (written {ref[2]:.1e}, bound {vc.VALUE_LOSS_BOUND:.1e})")
    assert worst[0] <= ref[0] and worst[1] <= ref[1] and worst[2] <= ref[2], (name, worst)


# ---- mutants --------------------------------------------------------------------------------------------------------------------
def _old_stats_accept(got, want, keys=vc.VALUE_STAT_KEYS):
    """The statistics assertions of tests/test_gpu_value_head.py as they stood: 1e-4 max(1, |want|), max / min equal where all five are checked."""
    with np.errstate(all="ignore"):
        close = all(abs(got[k] - want[k]) <= 1e-4 * max(1.0, abs(want[k])) for k in keys)
    return bool(close and (len(keys) < 5 or (got["value_max"] == want["value_max"] and got["value_min"] == want["value_min"])))


def _old_grad_accept(g, want_fp32, mask, shape):
    """Its gradient assertions: rtol 1e-5 against the fp32 oracle, zeros on unlabelled targets and in the last column."""
    g2, m2 = np.asarray(g, dtype=np.float64).reshape(shape), mask.reshape(shape)
    return bool(np.allclose(g2, np.asarray(want_fp32, dtype=np.float64).reshape(shape), rtol=1e-5, atol=1e-12)
                and not g2[:, :-1][~m2[:, :-1]].any() and not g2[:, -1].any())


# mutant -> do the suite's earlier assertions, evaluated on the same arrays, accept it?  (asserted below, so this table cannot go stale)
OLD_ACCEPTS = {
    "prediction paired across the row boundary": False,        # rejected on these arrays, but no kernel-level case had rows > 1
    "non-zero gradient in the last column": False,             # checked for row 0 only (`g_val[0, -1]`): a later row's passes
    "a label in column 0 counted": False,
    "the overlong factor missing from w": False,
    "gradient x 1.0003": False,                                # rtol 1e-5 sees it; the 1e-4 max norm of the goldens would not
    "the 0.5 applied to the gradient": False,
    "gradient of element 262144 zeroed": False,                # rejected on these arrays; the largest case had 65 536 entries
    "a NaN dropped from value_max": True,                      # only value_loss / value_mse / value_mean were looked at
    "value_mean with the neighbour's num_labels at a segment start": False,  # 8e-3 of the terms on a 257-token row; invisible only to a long row
    "unlabelled tokens entering value_mse": False,
    "an overflowed sequence left out of value_mean": False,
    "the no-label batch reporting -inf / +inf for max / min": False,
}
SEEN = set()


def _verdict(label, new_ok, score, bound, old_accepts):
    print(f"mutant '{label}': scores {score:.3e} against the bound {bound:.1e}; the earlier assertions {'accept' if old_accepts else 'reject'} it")
    assert not new_ok, label
    assert old_accepts == OLD_ACCEPTS[label], label
    SEEN.add(label)


def _correct(w):
    """A correct fp32 result: the witness rounded once."""
    return w.grad.astype(F32), dict(w.stats)


def test_mutants_of_the_pairing_are_rejected():
    b, value = ve.build(7, 64)
    cfg = ve.value_cfg(True, True)
    w = vc.witness(cfg, value=value, **vc.columns(b))
    g, stats = _correct(w)
    _, g32, s32 = vc.oracle_fp32(cfg, b, value)
    assert vc.check_grad(g, w).ok() and vc.check_stats(stats, w).ok() and _old_grad_accept(g, g32, w.mask, w.shape) and _old_stats_accept(stats, s32)

    wrong = vc.witness(cfg, value=value, **vc.columns(b), mutate="flat_shift")
    rg, rs = vc.check_grad(wrong.grad.astype(F32), w), vc.check_stats(wrong.stats, w)
    assert rg.stray > 0 and rg.stray_at % 64 == 63 and not rs.ok()
    _verdict("prediction paired across the row boundary", rg.ok() or rs.ok(), float(rg.stray), 0.0,
             _old_grad_accept(wrong.grad, g32, w.mask, w.shape) or _old_stats_accept(wrong.stats, s32))

    m = g.copy()
    m[3 * 64 - 1] = F32(1e-3)
    rg = vc.check_grad(m, w)
    assert rg.stray == 1 and rg.stray_at == 191
    old_row0_only = bool(np.allclose(m, g32, rtol=1e-5, atol=1e-12)) or m.reshape(7, 64)[0, -1] == 0  # what the earlier test looked at: row 0
    assert old_row0_only
    _verdict("non-zero gradient in the last column", rg.ok(), 1.0, 0.0, _old_grad_accept(m, g32, w.mask, w.shape))

    lab0 = b["labels"][:, 0] != -100
    assert lab0.sum() >= 6
    with np.errstate(all="ignore"):
        extra = float(np.nan_to_num(value[lab0, 0].astype(np.float64) / np.maximum(b["num_labels"][lab0, 0], 1)).sum())
    mstats = dict(stats, value_mean=stats["value_mean"] + extra)
    rs = vc.check_stats(mstats, w)
    _verdict("a label in column 0 counted", rs.ok(), rs.err, vc.VALUE_STAT_BOUND, _old_stats_accept(mstats, s32))

    wrong = vc.witness(cfg, value=value, **vc.columns(b), mutate="no_overflow")
    rg = vc.check_grad(wrong.grad.astype(F32), w)
    assert rg.stray > 10
    _verdict("the overlong factor missing from w", rg.ok(), float(rg.stray), 0.0, _old_grad_accept(wrong.grad, g32, w.mask, w.shape))


def test_mutants_of_the_gradient_are_rejected():
    b, value = ve.build(3, 87383)
    cfg = ve.value_cfg()
    w = vc.witness(cfg, value=value, **vc.columns(b))
    g, _ = _correct(w)
    _, g32, _ = vc.oracle_fp32(cfg, b, value)
    assert vc.check_grad(g, w).ok() and vc.check_grad(g, w).err <= 2.0 ** -23 and _old_grad_accept(g, g32, w.mask, w.shape)
    live = np.flatnonzero(w.scale > 0)
    u = int(live[np.argmax(np.abs(w.grad[live]) / w.scale[live])])  # an entry whose terms do not cancel (reward 0): the factor shows in full
    m = g.copy()
    m[u] *= F32(1.0003)
    rg = vc.check_grad(m, w)
    assert rg.at == u and rg.err > 2.9e-4
    _verdict("gradient x 1.0003", rg.ok(), rg.err, vc.VALUE_GRAD_BOUND, _old_grad_accept(m, g32, w.mask, w.shape))
    wrong = vc.witness(cfg, value=value, **vc.columns(b), mutate="half")
    rg = vc.check_grad(wrong.grad.astype(F32), w)
    _verdict("the 0.5 applied to the gradient", rg.ok(), rg.err, vc.VALUE_GRAD_BOUND, _old_grad_accept(wrong.grad, g32, w.mask, w.shape))
    m = g.copy()
    assert m[ve.ROUND] != 0
    m[ve.ROUND] = 0
    rg = vc.check_grad(m, w)
    assert rg.at == ve.ROUND and rg.err > 1e-3
    _verdict("gradient of element 262144 zeroed", rg.ok(), rg.err, vc.VALUE_GRAD_BOUND, _old_grad_accept(m, g32, w.mask, w.shape))


def test_mutants_of_the_statistics_are_rejected():
    cfg = ve.value_cfg(True, True)
    # a NaN prediction on a labelled token
    b, value, i = ve.poisoned("nan", True, ve.NONFINITE_SHAPES[0])
    w = vc.witness(cfg, value=value, **vc.columns(b))
    with np.errstate(all="ignore"):
        _, _, s32 = vc.oracle_fp32(cfg, b, value)
    assert np.isnan(w.stats["value_max"]) and np.isnan(w.stats["value_min"]) and np.isnan(s32["value_max"])
    stats = dict(w.stats, value_max=float(np.nanmax(value.reshape(-1)[w.mask])))  # what fmaxf leaves
    rs = vc.check_stats(stats, w)
    assert rs.mismatch == ["value_max"]
    _verdict("a NaN dropped from value_max", rs.ok(), np.inf, 0.0, _old_stats_accept(stats, s32, keys=("value_loss", "value_mse", "value_mean")))

    # sums, on the packed row whose only labels sit on the segment boundaries and on a dense one
    for shape, sparse in (((1, 1001), True), ((1, 257), False)):
        b, value = ve.build(*shape, seed=3, sparse=sparse)
        w = vc.witness(cfg, value=value, **vc.columns(b))
        _, _, s32 = vc.oracle_fp32(cfg, b, value)
        assert vc.check_stats(dict(w.stats), w).ok() and _old_stats_accept(w.stats, s32)
        results = {}
        for label, mutate in (("value_mean with the neighbour's num_labels at a segment start", "neighbour_num_labels"),
                              ("unlabelled tokens entering value_mse", "unlabelled_mse"),
                              ("an overflowed sequence left out of value_mean", "skip_overflow_mean")):
            wrong = vc.witness(cfg, value=value, **vc.columns(b), mutate=mutate)
            rs = vc.check_stats(wrong.stats, w)
            assert not rs.ok() and rs.err > 1e-3, (label, shape, str(rs))
            results[label] = (rs, _old_stats_accept(wrong.stats, s32))
            print(f"  {shape} sparse={sparse}: '{label}' scores {rs.err:.3e}; the earlier assertions {'accept' if results[label][1] else 'reject'} it")
        if not sparse:  # the dense row is the kind of case the suite had
            for label, (rs, old) in results.items():
                _verdict(label, rs.ok(), rs.err, vc.VALUE_STAT_BOUND, old)

    b, value = ve.no_label_batch(ve.NONFINITE_SHAPES[0])
    w = vc.witness(cfg, value=value, **vc.columns(b))
    stats = dict(w.stats, value_max=-np.inf, value_min=np.inf)
    rs = vc.check_stats(stats, w)
    assert sorted(rs.mismatch) == ["value_max", "value_min"] and list(w.stats.values()) == [0.0] * 5
    _verdict("the no-label batch reporting -inf / +inf for max / min", rs.ok(), np.inf, 0.0, _old_stats_accept(stats, {k: 0.0 for k in vc.VALUE_STAT_KEYS}))


def test_every_mutant_of_the_issue_was_tried():
    assert SEEN == set(OLD_ACCEPTS), sorted(set(OLD_ACCEPTS) - SEEN)


def test_guard_refuses_an_element_next_to_flt_max():
    b, value = ve.build(1, 257)
    b = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in b.items()}
    cfg = ve.value_cfg()  # w = 1 / 16
    i = int(np.flatnonzero((b["labels"][0, 1:] != -100) & (b["rewards"][0, 1:] == 0))[4])
    value = value.copy()
    value[0, i] = F32(np.sqrt(vc.FLT_MAX))  # (v - r)^2 within 2^-24 of FLT_MAX
    with pytest.raises(vc.BadCase, match=f"entry {i}"):
        vc.witness(cfg, value=value, **vc.columns(b))
    vc.witness(cfg, value=value, **vc.columns(b), guard=False)
    value[0, i] = F32(0.9 * np.sqrt(vc.FLT_MAX))
    assert vc.witness(cfg, value=value, **vc.columns(b)).finite[i]
    b["labels"][0, i + 1] = -100  # on an unlabelled target nothing hangs on the decision: accepted
    value[0, i] = F32(np.sqrt(vc.FLT_MAX))
    vc.witness(cfg, value=value, **vc.columns(b))
