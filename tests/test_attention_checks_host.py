"""tests/attention_checks.py checked on the host (no kernel runs here): the fp64 witness against a per-sequence loop, the
reference figures behind the bounds re-measured, the metric shown to catch a single wrong entry and a single leaked key, and the
CPU form of `segments()` against plain Python."""

import pytest
import torch

import attention_checks as ac
from pipelinerl_amd.fused_attention import BK, BQ, block_diagonal_mask, segments

CASES = ac.cases(BQ, BK)


@pytest.fixture(scope="module")
def problems():
    """case name -> (case, q, k, v, g, scale, seq_start, witness) at 4 query heads on 2 KV heads, D = 64; computed once."""
    out = {}
    for case in CASES:
        q, k, v, g, scale = ac.inputs(case, 4, 2, 64)
        ss, _ = ac.table_of(case.lengths)
        out[case.name] = (case, q, k, v, g, scale, ss, ac.witness(q, k, v, g, ss, scale))
    return out


def test_case_family_reaches_the_edges():
    b = max(BQ, BK)
    assert max(c.n for c in CASES) == 3 * b + 1
    edges = next(c for c in CASES if c.name == "edges")
    bounds = {sum(edges.lengths[:i]) for i in range(1, len(edges.lengths))}
    assert {b - 1, b, b + 1} <= bounds and any(x % b not in (0, 1, b - 1) for x in bounds)
    ones = next(c for c in CASES if c.name == "ones")
    assert ones.lengths[0] == 1 and ones.lengths[-1] == 1 and 1 in ones.lengths[1:-1]


def test_witness_agrees_with_the_per_sequence_loop(problems):
    for name, (case, q, k, v, g, scale, ss, wit) in problems.items():
        nv = ac.naive(q, k, v, g, case.lengths, scale)
        for out in ac.OUTPUTS:
            res = ac.measure(out, nv[out], wit[out][0], wit[out][1], 0.0)
            print(f"[attention] witness vs loop, {name}: {res}")
            assert res.stray == 0 and res.err < 1e-9, (name, str(res))


def test_long_case_moves_the_running_maximum_in_every_key_block(problems):
    case, q, k, v, g, scale, ss, wit = problems["long"]
    s = scale * torch.einsum("ihd,jhd->hij", q.double(), k.double().repeat_interleave(2, dim=1))
    row = s[0, case.n - 1]  # the last query sees every key block
    tops = [row[b0:b0 + BK].max().item() for b0 in range(0, case.n - 1, BK)]
    assert len(tops) >= 3 and tops[0] < tops[1] < tops[2], tops
    assert s.abs().max() >= 60.0


def test_reference_figures_are_what_the_table_says():
    """ATTN_REF is the reference op sequence's own error, re-measured: not above the table, and the table not above twice it."""
    for case in CASES:
        worst = {out: 0.0 for out in ac.OUTPUTS}
        ss, _ = ac.table_of(case.lengths)
        for d in ac.HEAD_SIZES:
            for hq, hkv in ac.HEADS:
                q, k, v, g, scale = ac.inputs(case, hq, hkv, d)
                wit = ac.witness(q, k, v, g, ss, scale)
                ref = ac.reference(q, k, v, g, ss, scale)
                for out in ac.OUTPUTS:
                    res = ac.measure(out, ref[out], wit[out][0], wit[out][1], ac.rounding(out))
                    assert res.stray == 0, (case.name, str(res))
                    worst[out] = max(worst[out], res.err)
        print(f"[attention] reference, {case.name}: " + ", ".join(f"{o} {e:.3e}" for o, e in worst.items()))
        for out in ac.OUTPUTS:
            assert 0.5 * ac.ATTN_REF[case.name][out] <= worst[out] <= ac.ATTN_REF[case.name][out], (case.name, out, worst[out])


def test_metric_flags_a_single_wrong_entry(problems):
    case, q, k, v, g, scale, ss, wit = problems["edges"]
    for out in ac.OUTPUTS:
        want, size = wit[out]
        got = want.clone()
        ac.check_outputs(case.name, "exact", {out: got}, wit, verbose=False)
        at = tuple(s // 2 for s in want.shape)
        got[at] += 2.0 * ac.bound(case.name, out) * size[at] + ac.rounding(out) * want[at].abs()
        with pytest.raises(AssertionError):
            ac.check_outputs(case.name, "one wrong entry", {out: got}, wit, verbose=False)
    # a value where the witness has none (scale 0) is flagged whatever its size
    want, size = wit["out"]
    stray = ac.measure("out", torch.cat([want, torch.full_like(want[:1], 1e-30)]), torch.cat([want, torch.zeros_like(want[:1])]),
                       torch.cat([size, torch.zeros_like(size[:1])]))
    assert stray.stray == want[:1].numel() and not stray.ok(1.0)


def test_metric_flags_a_leaked_key(problems):
    """One extra visible key across a boundary - the first query of a sequence also sees the last key of the sequence before."""
    for name in ("edges", "b2"):
        case, q, k, v, g, scale, ss, wit = problems[name]
        starts = sorted({int(x) for x in ss.tolist()} - {0})
        assert starts
        for at in starts:
            leaky = ss.clone()
            leaky[at] = at - 1
            got = ac.witness(q, k, v, g, leaky, scale)
            flagged = [out for out in ac.OUTPUTS if not ac.measure(out, got[out][0], wit[out][0], wit[out][1], ac.rounding(out)).ok(ac.bound(name, out))]
            print(f"[attention] leak into token {at} of {name}: flagged by {flagged}")
            assert flagged, (name, at)


# ---- segments() on the CPU against plain Python ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ac.segment_cases()))
def test_segments_on_the_cpu_against_plain_python(name):
    pos, mask, (batch, t) = ac.segment_cases()[name]
    want = ac.plain_segments(pos, mask, batch, t)
    got = segments(None if pos is None else torch.tensor(pos), None if mask is None else torch.tensor(mask), (batch, t))
    assert got[0].dtype == torch.int32 and got[1].dtype == torch.int32
    assert got[0].tolist() == want[0] and got[1].tolist() == want[1]
    if mask is not None:  # a bool mask is the same mask
        again = segments(None if pos is None else torch.tensor(pos), torch.tensor(mask).bool())
        assert again[0].tolist() == want[0] and again[1].tolist() == want[1]


def test_block_diagonal_mask_is_the_table():
    pos, mask, (batch, t) = ac.segment_cases()["padding_with_positions"]
    ss, se = segments(torch.tensor(pos), torch.tensor(mask))
    dense = block_diagonal_mask(ss, batch, t)
    assert dense.shape == (batch, 1, t, t) and dense.dtype == torch.bool
    for b in range(batch):
        for i in range(t):
            for j in range(t):
                assert bool(dense[b, 0, i, j]) == (int(ss[b * t + i]) <= b * t + j <= b * t + i)
    assert all(int(se[i]) > i >= int(ss[i]) for i in range(batch * t))
