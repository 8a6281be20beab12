"""tests/attention_sp_checks.py checked on the host (no kernel runs here): the case family reaches the edges it names, the table
of bounds is the unsliced flash arithmetic's own error re-measured, the honest slice composition stays under the bounds on every
case, and the seeded mistakes of the composition are flagged (bf16-rounded partials: the measured factor is reported)."""

import pytest

import attention_checks as ac
import attention_sp_checks as sp
from pipelinerl_amd.fused_attention import BK, BQ, varlen_attention_slice  # noqa: F401  (the feature these checks belong to)


@pytest.fixture(scope="module")
def problems():
    """case name -> (case, q, k, v, g, scale, seq_start, witness) at 4 query heads on 2 KV heads, D = 64; computed once."""
    out = {}
    for case in sp.CASES:
        q, k, v, g, scale, ss, _ = sp.problem(case, 4, 2, 64)
        out[case.name] = (case, q, k, v, g, scale, ss, ac.witness(q, k, v, g, ss, scale))
    return out


def test_case_family_reaches_the_edges():
    cases = {c.name: c for c in sp.CASES}
    assert list(cases) == ["sp_aligned", "sp_unaligned", "sp_four", "sp_long"] and set(sp.ATTN_SP_FLASH) == set(cases)
    assert sp.TILE == BQ == BK and sp.HEADS == ((4, 2), (7, 1)) and sp.HEAD_SIZES == (64, 128)
    a = cases["sp_aligned"]
    assert (a.p, a.slice_len) == (2, 128) and a.slice_len % BK == 0 and a.lengths[0] < a.slice_len < a.n  # the second sequence crosses the cut
    u = cases["sp_unaligned"]
    assert (u.p, u.slice_len) == (2, 129) and u.slice_len % BK and u.slice_len % 8
    ss = ac.table_of(u.lengths)[0].tolist()
    assert ss[u.slice_len] // BK * BK < u.slice_len - BK  # rank 1's sweep starts well inside rank 0's keys
    f = cases["sp_four"]
    assert (f.p, f.slice_len) == (4, 96) and f.lengths[0] == f.slice_len and 1 in f.lengths
    ss, se = (t.tolist() for t in ac.table_of(f.lengths))
    assert ss[96] == 96 and any(se[i] - ss[i] == 199 and ss[i] // 96 + 2 == (se[i] - 1) // 96 for i in range(f.n))  # one sequence on three ranks
    lg = cases["sp_long"]
    assert (lg.p, lg.slice_len, lg.lengths) == (4, 96, (384,)) and lg.ramp and lg.score == 20.0


def test_long_case_reaches_scores_of_60(problems):
    import torch

    case, q, k, v, g, scale, ss, wit = problems["sp_long"]
    s = scale * torch.einsum("ihd,jhd->hij", q.double(), k.double().repeat_interleave(2, dim=1))
    assert s.abs().max() >= 60.0


def test_table_is_the_unsliced_flash_arithmetic_re_measured():
    for case in sp.CASES:
        worst = {out: 0.0 for out in ac.OUTPUTS}
        for d in sp.HEAD_SIZES:
            for hq, hkv in sp.HEADS:
                q, k, v, g, scale, ss, _ = sp.problem(case, hq, hkv, d)
                wit = ac.witness(q, k, v, g, ss, scale)
                got = ac.flash_reference(q, k, v, g, ss, scale)
                for out in ac.OUTPUTS:
                    res = ac.measure(out, got[out], wit[out][0], wit[out][1], ac.rounding(out))
                    assert res.stray == 0, (case.name, str(res))
                    worst[out] = max(worst[out], res.err)
        print(f"[attention sp] flash arithmetic, whole row, {case.name}: " + ", ".join(f"{o} {e:.3e}" for o, e in worst.items()))
        for out in ac.OUTPUTS:
            table = sp.ATTN_SP_FLASH[case.name][out]
            figure = max(worst[out], ac.LSE_FLOOR) if out == "lse" else worst[out]
            assert 0.5 * table <= figure <= table, (case.name, out, worst[out])


def test_honest_composition_passes_every_case_at_every_head_shape():
    for case in sp.CASES:
        for d in sp.HEAD_SIZES:
            for hq, hkv in sp.HEADS:
                q, k, v, g, scale, ss, _ = sp.problem(case, hq, hkv, d)
                got = sp.sp_compose(q, k, v, g, ss, scale, case.p)
                sp.check_outputs(case.name, f"sp_compose {case.name} {hq}/{hkv} heads d {d}", got, ac.witness(q, k, v, g, ss, scale))


def test_one_slice_is_the_unsliced_arithmetic_bit_for_bit(problems):
    """P = 1: the composition is `flash_reference` itself - the slice form adds nothing but the offset and the fold."""
    import torch

    for name, (case, q, k, v, g, scale, ss, wit) in problems.items():
        a, b = sp.sp_compose(q, k, v, g, ss, scale, 1), ac.flash_reference(q, k, v, g, ss, scale)
        for out in ac.OUTPUTS:
            assert torch.equal(a[out], b[out]), (name, out)


@pytest.fixture(scope="module")
def seeded(problems):
    table = {}
    for mistake, switches in sp.MISTAKES.items():
        table[mistake] = {}
        for name, (case, q, k, v, g, scale, ss, wit) in problems.items():
            got = sp.sp_compose(q, k, v, g, ss, scale, case.p, **switches)
            res = {out: ac.measure(out, got[out], wit[out][0], wit[out][1], ac.rounding(out)) for out in ac.OUTPUTS}
            table[mistake][name] = {out: (float("inf") if r.stray else r.err) for out, r in res.items()}
    return table


def flagged(errs: dict, case: str) -> list:
    return [out for out in ac.OUTPUTS if not errs[out] <= sp.bound(case, out)]


def test_seeded_mistakes_are_flagged(seeded):
    assert list(sp.MISTAKES) == ["offset_dropped", "restart_at_cut", "rank_left_out", "parts_bf16"]
    caught = {}
    for mistake in sp.MISTAKES:
        caught[mistake] = []
        for name, errs in seeded[mistake].items():
            ratio, out = max((errs[o] / sp.bound(name, o), o) for o in ac.OUTPUTS)
            print(f"[attention sp] {mistake}, {name}: worst {out} {errs[out]:.3e} = {ratio:.3g} x bound, flagged {flagged(errs, name)}")
            if flagged(errs, name):
                caught[mistake].append(name)
    for mistake in ("offset_dropped", "restart_at_cut", "rank_left_out"):
        assert caught[mistake], mistake
    # a left-out rank shows in dk / dv only: out, lse and dq of every slice are final
    for name, errs in seeded["rank_left_out"].items():
        assert set(flagged(errs, name)) == {"dk", "dv"}, (name, flagged(errs, name))
    # bf16-rounded partials: one more rounding per rank on dk / dv.  Measured here at 0.2 - 0.3 x the bound with P = 2 .. 4: the
    # per-entry bounds do not see it (DESIGN.md section 3c says so); the fp32 partials are a choice of arithmetic the bit-for-bit
    # one-part fold test pins on the GPU, not something these bounds enforce.  Should a CPU flag it, it must be on dk / dv.
    for name in caught["parts_bf16"]:
        assert set(flagged(seeded["parts_bf16"][name], name)) <= {"dk", "dv"}
    worst = max(seeded["parts_bf16"][n][o] / sp.bound(n, o) for n in seeded["parts_bf16"] for o in ("dk", "dv"))
    print(f"[attention sp] parts_bf16: worst dk / dv {worst:.3g} x bound, flagged on {caught['parts_bf16'] or 'no case'}")


def test_bf16_partials_add_error_to_dk_dv(problems):
    """What the bounds do not see is still there: with the partials rounded to bf16 before the fold, dk / dv of a case whose keys
    get terms from several ranks differ from the single-rounding result, and never on out, lse, dq."""
    import torch

    case, q, k, v, g, scale, ss, wit = problems["sp_long"]
    a = sp.sp_compose(q, k, v, g, ss, scale, case.p)
    b = sp.sp_compose(q, k, v, g, ss, scale, case.p, parts_bf16=True)
    for out in ("out", "lse", "dq"):
        assert torch.equal(a[out], b[out])
    assert not torch.equal(a["dk"], b["dk"]) and not torch.equal(a["dv"], b["dv"])
    # rank 0's keys get terms from all four ranks; the last rank's keys from one: there the two agree
    tail = slice(3 * case.slice_len, case.n)
    assert torch.equal(a["dk"][tail], b["dk"][tail]) and torch.equal(a["dv"][tail], b["dv"][tail])
