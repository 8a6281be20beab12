"""K5 (`seq_scan_kernel`, `group_adv_kernel` of csrc/prl_pack.hip, through the C ABI `prl_seq_scan` / `prl_group_advantages`) against
plain Python, on the kernels' own edges.  K5 produces `advantages` (without a value head), `group_tokens`, `num_labels` and `overflow`:
the inputs of every token weight.  The suite compared it with the oracle on fewer than 60 random sequences and on 8 attempts per group.

`group_adv_kernel` walks a (group, step) key in chunks of one wave of 64: keys of 1, 2, 3, 63, 64, 65, 127, 128, 129 and 200 members in
one launch reach the single partial chunk, the exactly full one, the second chunk and a partial last one; members of different keys
interleaved in dataset order, two steps per group (keys != groups), rollout indices shared by several members (rollouts < members);
a second launch with 700 keys of 1 .. 5 members.  Checks: `group_tokens64` = Python's integer sum / rollout count exactly; the fp32
outputs are the casts of the fp64 ones bit for bit; a key whose rewards are all the same multiple of 1 / 8 has advantage exactly 0 at
every size (the zero-advantage group mask depends on it); for normal rewards |got - witness| / ((|r| + |loo|) / (sd + 1e-4)) (without
the divisor when the division by the std is off) against a long-double witness, under 4 x the same metric of
`oracle.preprocess.sequence_scalars` (math.fsum), measured on the CPU: ADV_REF, re-measured by the CPU test at the end of this file.

`seq_scan_kernel` reads a sequence as an unaligned head, a body of 16-byte loads and a tail, and falls back to element loads when no
aligned quad lies inside the sequence or a base pointer is not 16-byte aligned.  Sequences of 1 .. 4099 tokens whose starts and ends
take every residue mod 4, the only label / the only EOS on the first and on the last element and on both sides of the body's two
ends, the finish table {none, length, stop} x finished x EOS present, 4397 short sequences in one launch (workgroups loop over
sequences), and the same arrays handed over as views one element off (the fallback): all exact against plain Python.

Defect found by `sizes`: the key sums were plain left-to-right double sums; on the 200-member key that scored 1.58e-15 (std) /
1.42e-15 (no std) against the bound of 1.24e-15 - to the last digit the figure of the same plain sum evaluated on the host, so chunking,
the partial last chunk and the interleaving were right and the miss was the summation itself: a few ulp of the partial sums, kept by the
leave-one-out mean against the member's own small terms, where the oracle's math.fsum (and the reference's compensated pandas group sum)
is exact.  `ordered_wave_sum` is now a compensated (Neumaier) sum in the same dataset order; evaluated on the host it scores what the
oracle scores (3.1e-16)."""

import functools

import numpy as np
import pytest
import torch

from oracle import preprocess as opre

KEY_SIZES = (1, 2, 3, 63, 64, 65, 127, 128, 129, 200)
SCAN_LENS = (1, 2, 3, 4, 5, 7, 8, 255, 256, 257, 1023, 1024, 1025, 4099)
EOS = 2
# |adv - witness| / ((|r| + |loo|) / (sd + 1e-4)) of oracle.preprocess.sequence_scalars over both group cases and both settings of
# divide_advantage_by_std, measured on the CPU, rounded up to two digits
ADV_REF = 3.1e-16
ADV_BOUND = 4.0 * ADV_REF


# ---- group_adv_kernel: cases and the plain-Python witness (host code) ------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def group_case(name, rewards):
    """dict of per-sequence numpy arrays in dataset order: group_index, step_index, rollout_index, length, reward (fp64).
    `name`: "sizes" (KEY_SIZES as five groups x two steps, interleaved by a fixed permutation) or "many" (700 groups of 1 .. 5, one
    step).  `rewards`: "normal" or "dyadic" (every member of a key the same multiple of 1 / 8)."""
    rng = np.random.default_rng(41 if name == "sizes" else 43)
    if name == "sizes":
        keys = [(k // 2, k % 2, n) for k, n in enumerate(KEY_SIZES)]
    else:
        keys = [(g, 0, int(n)) for g, n in enumerate(rng.integers(1, 6, 700))]
    g = np.concatenate([np.full(n, gi) for gi, _, n in keys])
    st = np.concatenate([np.full(n, si) for _, si, n in keys])
    ro = np.concatenate([np.arange(n) // 2 for _, _, n in keys])  # two members per rollout, and both steps of a group share them
    key_id = np.concatenate([np.full(n, k) for k, (_, _, n) in enumerate(keys)])
    perm = rng.permutation(len(g))
    g, st, ro, key_id = g[perm], st[perm], ro[perm], key_id[perm]
    if rewards == "dyadic":
        r = (((key_id * 5) % 17) - 8) / 8.0
    else:
        r = rng.standard_normal(len(g))
    return dict(group_index=g.astype(np.int64), step_index=st.astype(np.int64), rollout_index=ro.astype(np.int64),
                length=rng.integers(1, 50, len(g)).astype(np.int64), reward=r.astype(np.float64), key_id=key_id)


def group_witness(case, divide_by_std):
    """(advantage [S] long double, scale [S] of the metric, group_tokens [S] as Python computes sum / count)."""
    S = len(case["reward"])
    by_key, rollout_tokens = {}, {}
    for s in range(S):
        by_key.setdefault((int(case["group_index"][s]), int(case["step_index"][s])), []).append(s)
        rk = (int(case["group_index"][s]), int(case["rollout_index"][s]))
        rollout_tokens[rk] = rollout_tokens.get(rk, 0) + int(case["length"][s])
    per_group = {}
    for (gi, _), n in rollout_tokens.items():
        per_group.setdefault(gi, []).append(n)
    adv, scale, gt = np.zeros(S, dtype=np.longdouble), np.zeros(S, dtype=np.longdouble), np.zeros(S, dtype=np.float64)
    LD = np.longdouble
    for members in by_key.values():
        rs = np.asarray([case["reward"][s] for s in members], dtype=LD)
        n = len(members)
        total = rs.sum()  # 64-bit mantissa: 2^-11 of a double's rounding per addition
        sd = LD(0)
        if n > 1:
            mean = total / LD(n)
            sd = np.sqrt(((rs - mean) ** 2).sum() / LD(n - 1))
        for s, r in zip(members, rs):
            loo = (total - r) / LD(n - 1) if n > 1 else r
            div = (sd + LD(1e-4)) if divide_by_std else LD(1)
            adv[s] = (r - loo) / div
            scale[s] = (abs(r) + abs(loo)) / div
    for s in range(S):
        toks = per_group[int(case["group_index"][s])]
        gt[s] = sum(toks) / len(toks)
    return adv, scale, gt


def adv_error(got, case, divide_by_std):
    adv, scale, _ = group_witness(case, divide_by_std)
    err = np.abs(np.asarray(got, dtype=np.longdouble) - adv)
    live = scale > 0
    assert not err[~live].any()
    return float((err[live] / scale[live]).max())


def oracle_entries(case):
    return [dict(group_id=int(case["group_index"][s]), step_index=int(case["step_index"][s]), rollout_index=int(case["rollout_index"][s]),
                 rewards=[float(case["reward"][s])], input_ids=[5] * int(case["length"][s]), labels=[5] * int(case["length"][s]), finished=True)
            for s in range(len(case["reward"]))]


# ---- seq_scan_kernel: cases and plain Python (host code) --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scan_case(name):
    """(tokens int32 [T], labels int32 [T], seq_off int64 [S + 1], finish_code uint8 [S], finished uint8 [S]).  "edges": every length of
    SCAN_LENS in six variants (below) and the finish table; "many": 4097 + 300 sequences of 1 .. 3 tokens."""
    from pipelinerl_amd import _lib

    rng = np.random.default_rng(47)
    if name == "many":
        lens = rng.integers(1, 4, 4097 + 300).tolist()
        variants = [None] * len(lens)
        table = []
    else:
        # 1-token spacers (variant None) shift the offsets so that long sequences start and end on every residue mod 4
        lens, variants = [], []
        for k, n in enumerate(SCAN_LENS):
            for v in range(6):
                lens.append(n)
                variants.append(v)
                if (k + v) % 3 == 0:
                    lens.append(1)
                    variants.append(None)
        table = [(code, fin, has) for code in (_lib.PRL_FINISH_NONE, _lib.PRL_FINISH_LENGTH, _lib.PRL_FINISH_STOP) for fin in (0, 1) for has in (0, 1)]
        lens += [9] * len(table)
        variants += [None] * len(table)
    S = len(lens)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    tokens = np.full(off[-1], 5, dtype=np.int32)
    labels = np.full(off[-1], -100, dtype=np.int32)
    code, fin = np.zeros(S, dtype=np.uint8), np.zeros(S, dtype=np.uint8)
    for s in range(S):
        b, e = int(off[s]), int(off[s + 1])
        a0, a1 = (b + 3) & ~3, e & ~3
        inside = lambda p, alt: p if b <= p < e else alt  # noqa: E731
        v = variants[s]
        if v is None and name == "many":
            if rng.random() < 0.5:
                labels[rng.integers(b, e)] = 7
            if rng.random() < 0.5:
                tokens[rng.integers(b, e)] = EOS
        elif v is not None:
            lab_at, eos_at = [(b, b), (e - 1, e - 1), (inside(a0 - 1, b), inside(a0, e - 1)), (inside(a0, e - 1), inside(a0 - 1, b)),
                              (inside(a1 - 1, b), inside(a1, e - 1)), (inside(a1, e - 1), inside(a1 - 1, b))][v]
            labels[lab_at] = 7
            tokens[eos_at] = EOS
    for k, (c, f, has) in enumerate(table):
        s = S - len(table) + k
        code[s], fin[s] = c, f
        labels[off[s] + 2:min(off[s] + 2 + k, off[s + 1])] = 7  # 0 .. 7 labels, nothing to do with the table
        if has:
            tokens[off[s] + 4] = EOS
    return tokens, labels, off, code, fin


def scan_expected(tokens, labels, off, code, fin):
    """reference rl/__init__.py:541-556 in plain Python: (num_labels, overflow) per sequence."""
    from pipelinerl_amd import _lib

    nl, ov = [], []
    for s in range(len(off) - 1):
        t, lab = tokens[off[s]:off[s + 1]].tolist(), labels[off[s]:off[s + 1]].tolist()
        nl.append(float(sum(1 for x in lab if x != -100)))
        if code[s] == _lib.PRL_FINISH_LENGTH:
            ov.append(1.0)
        elif code[s] == _lib.PRL_FINISH_STOP or fin[s]:
            ov.append(0.0)
        else:
            ov.append(0.0 if EOS in t else 1.0)
    return nl, ov


# ---- GPU tests ------------------------------------------------------------------------------------------------------------------
def run_group(lib, dev, case, divide_by_std):
    from pipelinerl_amd import _lib
    from pipelinerl_amd.finetune.rl import plan_groups, upload_packed

    S = len(case["reward"])
    plan = upload_packed(plan_groups(case["group_index"], case["step_index"], case["rollout_index"]), dev)
    off = torch.from_numpy(np.concatenate([[0], np.cumsum(case["length"])]).astype(np.int64)).to(dev)
    reward = torch.from_numpy(case["reward"]).to(dev)
    out64 = torch.full((2, S), float("nan"), dtype=torch.float64, device=dev)
    out32 = torch.full((2, S), float("nan"), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.prl_group_advantages(S, len(plan[0]) - 1, len(plan[2]) - 1, *[_lib.ptr(p) for p in plan], _lib.ptr(reward), _lib.ptr(off),
                                            int(divide_by_std), _lib.ptr(out64[0]), _lib.ptr(out64[1]), _lib.ptr(out32[0]), _lib.ptr(out32[1]),
                                            _lib.current_stream_ptr(dev)))
    torch.cuda.synchronize(dev)
    return out64.cpu().numpy(), out32.cpu().numpy(), (len(plan[0]) - 1, len(plan[2]) - 1)


@pytest.mark.gpu
@pytest.mark.parametrize("divide_by_std", [True, False], ids=["std", "no_std"])
@pytest.mark.parametrize("name", ["sizes", "many"])
def test_group_advantages(libprl, cuda_device, name, divide_by_std):
    for rewards in ("normal", "dyadic"):
        case = group_case(name, rewards)
        out64, out32, (n_keys, n_groups) = run_group(libprl, cuda_device, case, divide_by_std)
        assert (n_keys, n_groups) == ((10, 5) if name == "sizes" else (700, 700))
        _, _, gt = group_witness(case, divide_by_std)
        assert np.array_equal(out64[1], gt), "group_tokens64 is not Python's sum / count"
        assert np.array_equal(out32[0].view(np.uint32), out64[0].astype(np.float32).view(np.uint32)), "adv32 is not the cast of adv64"
        assert np.array_equal(out32[1].view(np.uint32), out64[1].astype(np.float32).view(np.uint32)), "gt32 is not the cast of gt64"
        if rewards == "dyadic":
            assert not out64[0].any() and not np.isnan(out64[0]).any(), "equal rewards in a key must give advantage exactly 0"
        else:
            err = adv_error(out64[0], case, divide_by_std)
            print(f"[k5] {name} divide_by_std={divide_by_std}: advantage {err:.3e} of (|r| + |loo|) / (sd + 1e-4) (reference {ADV_REF:.1e}, bound {ADV_BOUND:.1e})")
            assert err <= ADV_BOUND


def run_scan(lib, dev, arrays, offset_views=False):
    from pipelinerl_amd import _lib

    tokens, labels, off, code, fin = arrays
    S = len(off) - 1

    def put(a):
        t = torch.from_numpy(a).to(dev)
        if not offset_views:
            return t
        buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=dev)
        buf[1:] = t
        return buf[1:]
    tk, lb = put(tokens), put(labels)
    assert (tk.data_ptr() % 16 != 0) == offset_views and (lb.data_ptr() % 16 != 0) == offset_views
    d_off, d_code, d_fin = (torch.from_numpy(a).to(dev) for a in (off, code, fin))
    out = torch.full((2, S), float("nan"), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.prl_seq_scan(S, _lib.ptr(tk), _lib.ptr(lb), _lib.ptr(d_off), _lib.ptr(d_code), _lib.ptr(d_fin), EOS, _lib.ptr(out[0]),
                                    _lib.ptr(out[1]), _lib.current_stream_ptr(dev)))
    torch.cuda.synchronize(dev)
    o = out.cpu().numpy()
    return o[0].tolist(), o[1].tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["edges", "many"])
def test_seq_scan(libprl, cuda_device, name):
    arrays = scan_case(name)
    want = scan_expected(*arrays)
    got = run_scan(libprl, cuda_device, arrays)
    assert got[0] == want[0], "num_labels"
    assert got[1] == want[1], "overflow"
    again = run_scan(libprl, cuda_device, arrays, offset_views=True)  # base pointers 4 bytes off 16-byte alignment: the element-load fallback
    assert again == got


# ---- CPU: the cases are what they claim, and the yardstick of ADV_BOUND ----------------------------------------------------------
def test_group_cases_and_the_oracle_reference():
    worst = 0.0
    for name in ("sizes", "many"):
        case = group_case(name, "normal")
        keys = {}
        for s in range(len(case["reward"])):
            keys.setdefault((case["group_index"][s], case["step_index"][s]), []).append(s)
        sizes = sorted(len(v) for v in keys.values())
        if name == "sizes":
            assert sizes == sorted(KEY_SIZES) and len({g for g, _ in keys}) == 5
            # interleaved: the members of the largest key are not contiguous in dataset order
            big = max(keys.values(), key=len)
            assert np.diff(big).max() > 1 and np.diff(big).min() >= 1
            pairs = {(g, r) for g, r in zip(case["group_index"], case["rollout_index"])}
            assert all(sum(1 for p in pairs if p[0] == g) < sum(len(v) for k, v in keys.items() if k[0] == g) for g in range(5))
        else:
            assert len(keys) == 700 and sizes[0] == 1 and sizes[-1] == 5
        data = oracle_entries(case)
        for divide_by_std in (True, False):
            want = opre.sequence_scalars(data, EOS, divide_by_std)
            _, _, gt = group_witness(case, divide_by_std)
            assert [w[1] for w in want] == gt.tolist()
            err = adv_error([w[0] for w in want], case, divide_by_std)
            print(f"oracle sequence_scalars {name} divide_by_std={divide_by_std}: {err:.3e} (written {ADV_REF:.1e})")
            worst = max(worst, err)
        dy = group_case(name, "dyadic")
        assert np.array_equal(dy["reward"] * 8, np.round(dy["reward"] * 8)) and len(set(dy["reward"])) > 5
        for divide_by_std in (True, False):
            assert all(w[0] == 0 for w in opre.sequence_scalars(oracle_entries(dy), EOS, divide_by_std))
            assert not group_witness(dy, divide_by_std)[0].any()
    assert worst <= ADV_REF


def test_scan_cases_reach_every_region_edge():
    tokens, labels, off, code, fin = scan_case("edges")
    lens = np.diff(off)
    assert set(SCAN_LENS) <= set(lens.tolist())
    long = lens >= 255
    assert {int(b) % 4 for b in off[:-1][long]} == {0, 1, 2, 3} and {int(e) % 4 for e in off[1:][long]} == {0, 1, 2, 3}
    assert {int(b) % 4 for b in off[:-1][~long]} == {0, 1, 2, 3}
    first_lab = last_lab = first_eos = last_eos = 0
    around = set()
    for s in range(len(lens) - 12):
        b, e = int(off[s]), int(off[s + 1])
        if lens[s] == 1 and (labels[b] == -100):
            continue  # a spacer
        lab, eos = np.flatnonzero(labels[b:e] != -100) + b, np.flatnonzero(tokens[b:e] == EOS) + b
        assert len(lab) == 1 and len(eos) == 1
        first_lab += lab[0] == b
        last_lab += lab[0] == e - 1
        first_eos += eos[0] == b
        last_eos += eos[0] == e - 1
        a0, a1 = (b + 3) & ~3, e & ~3
        if lens[s] >= 255:
            around.update(k for k, p in (("a0-1", a0 - 1), ("a0", a0), ("a1-1", a1 - 1), ("a1", a1)) if lab[0] == p and b <= p < e)
            around.update(k + " eos" for k, p in (("a0-1", a0 - 1), ("a0", a0), ("a1-1", a1 - 1), ("a1", a1)) if eos[0] == p and b <= p < e)
    assert min(first_lab, last_lab, first_eos, last_eos) >= len(SCAN_LENS)
    assert around == {k + suffix for k in ("a0-1", "a0", "a1-1", "a1") for suffix in ("", " eos")}
    nl, ov = scan_expected(tokens, labels, off, code, fin)
    assert ov[-12:] == [0.0 if (c == 2 or (c == 0 and (f or h))) else 1.0 for c in (0, 1, 2) for f in (0, 1) for h in (0, 1)] and nl[-12:] == [float(min(k, 7)) for k in range(12)]
    many = scan_case("many")
    assert len(many[2]) - 1 == 4097 + 300 > 4096 and set(np.diff(many[2]).tolist()) == {1, 2, 3}
    nl, ov = scan_expected(*many)
    assert 0.2 < np.mean(ov) < 0.8 and 0.2 < np.mean(nl) < 0.8
