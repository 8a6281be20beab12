"""tests/attention_checks.py checked on the host (no kernel runs here): the fp64 witness against a per-sequence loop, the
figures of both references (flash arithmetic: the bounds; eager bf16: their ceiling) re-measured, seeded mistakes of the flash
arithmetic shown to be caught by the bounds (and which of them the earlier, eager-based bounds let through), the metric shown to
catch a single wrong entry and a single leaked key, and the CPU form of `segments()` against plain Python."""

import math

import pytest
import torch

import attention_checks as ac
from pipelinerl_amd.fused_attention import BK, BQ, block_diagonal_mask, segments

CASES = ac.cases(BQ, BK)
OLD_CASES = ("edges", "ones", "long", "b2", "padded")  # the cases ATTN_REF has a row for


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
    assert max(c.n for c in CASES) == 4 * b + 1
    assert [c.name for c in CASES[:5]] == list(OLD_CASES) and len(CASES) == 12 and set(ac.ATTN_FLASH) == {c.name for c in CASES}
    edges = next(c for c in CASES if c.name == "edges")
    bounds = {sum(edges.lengths[:i]) for i in range(1, len(edges.lengths))}
    assert {b - 1, b, b + 1} <= bounds and any(x % b not in (0, 1, b - 1) for x in bounds)
    ones = next(c for c in CASES if c.name == "ones")
    assert ones.lengths[0] == 1 and ones.lengths[-1] == 1 and 1 in ones.lengths[1:-1]
    # "mid": some query block sweeps a first tile with its seq_start strictly inside it, then a tile wholly inside the sequence
    # and below the diagonal
    mid = next(c for c in CASES if c.name == "mid")
    ss = ac.table_of(mid.lengths)[0].tolist()
    found = []
    for q0 in range(0, mid.n, BQ):
        q1 = min(q0 + BQ, mid.n)
        lo, first_tile = ss[q0], ss[q0] // BK * BK
        whole = [k0 for k0 in range(first_tile + BK, q1, BK) if k0 >= ss[q1 - 1] and k0 + BK - 1 <= q0]
        if first_tile < lo < first_tile + BK and first_tile + BK <= q0 and whole:
            found.append((q0, first_tile, whole))
    assert found, "no query block of 'mid' starts its sweep inside a tile and goes on through a whole one"
    # the key block that holds the boundary sees whole query tiles of the second sequence only
    k0 = mid.lengths[0] // BK * BK
    assert k0 < mid.lengths[0] < k0 + BK and mid.n >= k0 + 3 * BK
    # two cases carry a scale that is not d ** -0.5, at both head sizes
    odd = [c.name for c in CASES if all(ac.inputs(c, 1, 1, d)[4] != d ** -0.5 for d in ac.HEAD_SIZES)]
    assert len(odd) == 2, odd
    for c in CASES:  # and every other case the usual one
        if c.name not in odd:
            assert all(ac.inputs(c, 1, 1, d)[4] == 1.0 / math.sqrt(d) for d in ac.HEAD_SIZES)


def test_scaled_cases_keep_the_score_distribution(problems):
    """The scaled cases' scores are those of the layouts they share to within the rounding of q to bf16."""
    for name, like in (("scaled", "edges"), ("scale_one", "b2")):
        _, q, k, _, _, scale, _, _ = problems[name]
        _, q0, k0, _, _, scale0, _, _ = problems[like]
        assert scale != scale0 and torch.equal(k, k0)
        s = scale * torch.einsum("ihd,jhd->hij", q.double(), k.double().repeat_interleave(2, dim=1))
        s0 = scale0 * torch.einsum("ihd,jhd->hij", q0.double(), k0.double().repeat_interleave(2, dim=1))
        assert (s - s0).abs().max() <= 2.0 ** -8 * scale0 * torch.einsum("ihd,jhd->hij", q0.abs().double(), k0.abs().double().repeat_interleave(2, dim=1)).max()


def test_flat_case_is_the_running_mean(problems):
    case, q, k, v, g, scale, ss, wit = problems["flat"]
    assert not q.any()
    want = torch.log((torch.arange(case.n) - ss.long() + 1).double())
    assert (wit["lse"][0] - want.view(1, -1)).abs().max() <= 1e-12
    i = case.n - 1
    mean = v[int(ss[i]):i + 1].double().mean(0).repeat_interleave(2, dim=0)
    assert (wit["out"][0][i] - mean).abs().max() <= 1e-12


def test_sink_case_gives_the_first_key_the_weight(problems):
    """The first key of a sequence is every row's maximum (more than half the weight) and on most rows holds nearly all of it: the
    maximum is set in the first swept tile and never moves."""
    case, q, k, v, g, scale, ss, wit = problems["sink"]
    s = scale * torch.einsum("ihd,jhd->hij", q.double(), k.double().repeat_interleave(2, dim=1)).masked_fill(~ac.visible(ss), float("-inf"))
    p_first = torch.exp(s[:, torch.arange(case.n), ss.long()] - wit["lse"][0])
    far = torch.arange(case.n) - ss.long() >= BK  # rows whose sweep goes past the first tile
    print(f"[attention] sink: weight of the first key, rows past the first tile: min {p_first[:, far].min():.4f} median {p_first[:, far].median():.6f}")
    assert far.any() and p_first[:, far].min() > 0.5 and p_first[:, far].median() > 0.999


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
    """ATTN_FLASH and ATTN_REF are the two references' own errors, re-measured: not above the table, and the table not above
    twice it (lse of the flash arithmetic: floored at LSE_FLOOR first).  The flash table - the bounds - is nowhere above the eager
    one: entry by entry for the cases ATTN_REF has, against the eager reference measured here (under the tables' rule) for the rest."""
    for case in CASES:
        flash = {out: 0.0 for out in ac.OUTPUTS}
        eager = {out: 0.0 for out in ac.OUTPUTS}
        ss, _ = ac.table_of(case.lengths)
        for d in ac.HEAD_SIZES:
            for hq, hkv in ac.HEADS:
                q, k, v, g, scale = ac.inputs(case, hq, hkv, d)
                wit = ac.witness(q, k, v, g, ss, scale)
                for worst, got in ((flash, ac.flash_reference(q, k, v, g, ss, scale)), (eager, ac.reference(q, k, v, g, ss, scale))):
                    for out in ac.OUTPUTS:
                        res = ac.measure(out, got[out], wit[out][0], wit[out][1], ac.rounding(out))
                        assert res.stray == 0, (case.name, str(res))
                        worst[out] = max(worst[out], res.err)
        print(f"[attention] flash arithmetic, {case.name}: " + ", ".join(f"{o} {e:.3e}" for o, e in flash.items()))
        print(f"[attention] eager reference, {case.name}: " + ", ".join(f"{o} {e:.3e}" for o, e in eager.items()))
        for out in ac.OUTPUTS:
            table = ac.ATTN_FLASH[case.name][out]
            figure = max(flash[out], ac.LSE_FLOOR) if out == "lse" else flash[out]
            assert 0.5 * table <= figure <= table, (case.name, out, flash[out])
            if case.name in ac.ATTN_REF:
                assert 0.5 * ac.ATTN_REF[case.name][out] <= eager[out] <= ac.ATTN_REF[case.name][out], (case.name, out, eager[out])
                assert table <= ac.ATTN_REF[case.name][out] and ac.bound(case.name, out) <= ac.old_bound(case.name, out)
            else:
                assert table <= ac.table_figure(eager[out], out), (case.name, out, eager[out])
    assert set(ac.ATTN_REF) == set(OLD_CASES)
    assert ac.bound("long", "out") < 0.1 and ac.bound("long", "dv") < 0.1


def test_table_rule():
    assert ac.table_figure(4.614e-3, "out") == pytest.approx(5.1e-3) and ac.table_figure(1.0e-3, "dq") == pytest.approx(1.1e-3)
    assert ac.table_figure(1e-9, "lse") == pytest.approx(6.6e-8) and ac.table_figure(0.0, "dk") == 0.0


# ---- seeded mistakes of the flash arithmetic ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def seeded(problems):
    """mistake (None: the honest arithmetic) -> case -> output -> the metric; every emulation runs once."""
    table = {}
    for mistake, switches in [(None, {})] + list(ac.MISTAKES.items()):
        table[mistake] = {}
        for name, (case, q, k, v, g, scale, ss, wit) in problems.items():
            got = ac.flash_reference(q, k, v, g, ss, scale, **switches)
            res = {out: ac.measure(out, got[out], wit[out][0], wit[out][1], ac.rounding(out)) for out in ac.OUTPUTS}
            table[mistake][name] = {out: (float("inf") if r.stray else r.err) for out, r in res.items()}
    return table


def flagged(errs: dict, case: str, limit) -> list:
    return [out for out in ac.OUTPUTS if not errs[out] <= limit(case, out)]


def test_honest_flash_arithmetic_passes_every_case(seeded):
    for name, errs in seeded[None].items():
        assert not flagged(errs, name, ac.bound), (name, errs)


def test_every_seeded_mistake_is_flagged_under_the_bounds(seeded):
    assert len(ac.MISTAKES) == 8
    for mistake in ac.MISTAKES:
        caught = []
        for name, errs in seeded[mistake].items():
            ratio, out = max((errs[o] / ac.bound(name, o) if ac.bound(name, o) else (float("inf") if errs[o] else 0.0), o) for o in ac.OUTPUTS)
            print(f"[attention] {mistake}, {name}: worst {out} {errs[out]:.3e} = {ratio:.3g} x bound, flagged {flagged(errs, name, ac.bound)}")
            if flagged(errs, name, ac.bound):
                caught.append(name)
        assert caught, mistake
    # a scale fixed at d ** -0.5 is invisible where that IS the scale
    for use in ac.SCALE_USES:
        caught = {name for name, errs in seeded[f"fixed_scale_{use}"].items() if flagged(errs, name, ac.bound)}
        assert caught == {"scaled", "scale_one"}, (use, caught)
    # the leaked tile needs a sequence that starts inside a block another query block lies past
    assert not flagged(seeded["whole_too_early"]["long"], "long", ac.bound)
    assert flagged(seeded["whole_too_early"]["mid"], "mid", ac.bound)


def test_what_the_eager_based_bounds_let_through(seeded):
    """Under the earlier bounds, 4 x ATTN_REF, on the cases they had: bf16 scores and a bf16 lse pass everything; a running sum
    that is never rescaled passes "long" - the one case that moves the maximum - on out and dv."""
    for mistake in ("scores_bf16", "lse_bf16"):
        for name in OLD_CASES:
            old = flagged(seeded[mistake][name], name, ac.old_bound)
            print(f"[attention] {mistake}, {name}: flagged under 4 x ATTN_REF {old}, under 4 x ATTN_FLASH {flagged(seeded[mistake][name], name, ac.bound)}")
            assert not old, (mistake, name, old)
    errs = seeded["sum_not_rescaled"]["long"]
    print("[attention] sum_not_rescaled, long: " + ", ".join(f"{o} {e:.3e} (old bound {ac.old_bound('long', o):.2e})" for o, e in errs.items()))
    assert errs["out"] <= ac.old_bound("long", "out") and errs["dv"] <= ac.old_bound("long", "dv")
    assert errs["out"] > ac.bound("long", "out") and errs["dv"] > ac.bound("long", "dv")


def test_scale_identity_holds_bit_for_bit_in_the_flash_arithmetic(problems):
    """scale -> 2 scale with q halved: the same scores bit for bit, so out, lse, dk and dv are the same bits and dq is exactly
    twice (what tests/test_gpu_attention.py asks of the kernels)."""
    case, q, k, v, g, scale, ss, wit = problems["b2"]
    a = ac.flash_reference(q, k, v, g, ss, scale)
    b = ac.flash_reference(0.5 * q, k, v, g, ss, 2.0 * scale)
    assert torch.equal(ac.bf16_exact(0.5 * q), 0.5 * q)
    for out in ("out", "lse", "dk", "dv"):
        assert torch.equal(a[out], b[out]), out
    assert torch.equal(2.0 * a["dq"], b["dq"])


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
