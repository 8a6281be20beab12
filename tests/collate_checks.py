"""Per-token check of pack collate (K6), padded collate (K7) and the OOV patch of csrc/prl_pack.hip (plain numpy; no kernel runs
here, nothing of the package is imported).

Why: these kernels build every training batch, and the suite held them to oracle parity on workload-shaped data only.  That never
launched the scalar-store form of K6 (`pack_collate_kernel<false, false, 4>`, taken when an output column is not 16-byte aligned),
gave the vector fast path long sequences only, never took a lane's second iteration (more than 1 048 576 lane groups), and never
placed a sequence start, a zero-length sequence or a filler on a workgroup's first token.

Witnesses (`pack_witness`, `pad_witness`, `oov_witness`) restate what oracle/preprocess.py states (`prepare_fields`,
`collate_packed`, `collate`, `sentinel_example`) over ragged arrays instead of example dicts:

    packed   position restarts at 0 in every packed sequence, segment = pk_seg, mask = 1; the label of token 0 is -100 whenever
             seg > 0; log-probs right-aligned in the sequence with zeros to their left; ref = old without reference log-probs; a
             filler (src < 0): ids = eos, labels -100, rewards 0, advantages 0, ref 0, old 0, group_tokens 1, num_labels 1, overflow 0
    padded   [n_rows, padded_len], padding ids 0, labels -100, mask 0, every fp32 column 0, on the right or on the left
    scalars  bit k of `per_token` reads column k of (rewards, advantages, group_tokens, num_labels, overflow) per token from a
             [T_src] array, otherwise per sequence from [S]; a filler's scalars ignore the bits
    oov      tokens outside [0, table_size) or with valid[token] == 0 become the_id; the count of those

Everything is integer work or copies: every comparison is exact, fp32 columns as their uint32 bit patterns (the inputs carry -0.0, a
denormal, +-inf and NaNs with a payload).  `pack_geometry` mirrors the launch arithmetic and is used only to PLACE edges and to NAME
the region of a mismatch, never to compute an expected value.
"""

from __future__ import annotations

import dataclasses
import functools

import numpy as np

I64_COLUMNS = ("input_ids", "labels", "attention_mask", "position_ids", "segment_ids")
F32_COLUMNS = ("rewards", "advantages", "ref_logprobs", "old_logprobs", "group_tokens", "num_labels", "overflow")
PACK_COLUMNS = I64_COLUMNS + F32_COLUMNS              # the C ABI's output order
PAD_COLUMNS = I64_COLUMNS[:3] + F32_COLUMNS
SCALAR_COLUMNS = ("rewards", "advantages", "group_tokens", "num_labels", "overflow")  # bit k of per_token_columns
ALL_BITS = 31
EOS = 2
INT32_MIN, INT32_MAX = -(2 ** 31), 2 ** 31 - 1

BLOCK = 256          # threads of a workgroup
MAX_BLOCKS = 4096    # the grid's cap
# a lane takes a second trip through its loop past BLOCK * MAX_BLOCKS = 1 048 576 lane groups (K6) or items (K7, patch_oov)
STRIDE_ITEMS = BLOCK * MAX_BLOCKS

CYCLE = (0, 1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 511, 512, 513)
EDGE_TOTAL = 12001   # odd; 24 workgroups of 251 pairs (aligned), 12 of 251 quads (unaligned)
# K6 "long".  Lane iterations = ceil(ceil(ngroups / 4096) / 256), ngroups = ceil(total / tokens per lane):
#   2 tokens per lane: 2 iterations past 2 097 152 tokens, 3 past 4 194 304;  4 tokens per lane: 2 past 4 194 304.
# Any total above 4 194 304 gives (3, 2); at 4 400 001 the last trip has 26 (pairs) / 13 (quads) lanes of every workgroup in it.
LONG_TOTAL = 4_400_001

# awkward fp32 bit patterns: -0.0, the smallest denormal, +inf, -inf, quiet NaNs with a payload (either sign)
AWKWARD_BITS = (0x80000000, 0x00000001, 0x7F800000, 0xFF800000, 0x7FC12345, 0xFFC54321)


# ---- geometry ---------------------------------------------------------------------------------------------------------------------
def pack_geometry(total: int, aligned: bool) -> tuple[int, int, int]:
    """(tokens per lane, workgroups, lane groups per workgroup) of one `prl_pack_collate` launch.  Mirrors `blocks_for` and the
    kernel's span split in csrc/prl_pack.hip: 2 tokens per lane when every output column is 16-byte aligned, else 4; 256 threads;
    ceil(ngroups / 256) workgroups, at most 4096; workgroup b owns lane groups [b * per_block, (b + 1) * per_block).  Used only to
    place and verify edges and to name regions, never to compute expected values."""
    tpl = 2 if aligned else 4
    ngroups = -(-total // tpl)
    n_blocks = min(max(-(-ngroups // BLOCK), 1), MAX_BLOCKS)
    return tpl, n_blocks, -(-ngroups // n_blocks)


def span_starts(total: int, aligned: bool) -> list[int]:
    """First token of every workgroup's span but the first (those that own at least one token)."""
    tpl, n_blocks, per_block = pack_geometry(total, aligned)
    return [b * per_block * tpl for b in range(1, n_blocks) if b * per_block * tpl < total]


def lane_iterations(total: int, aligned: bool) -> int:
    return -(-pack_geometry(total, aligned)[2] // BLOCK)


# ---- witnesses --------------------------------------------------------------------------------------------------------------------
def pack_witness(pk_src, pk_dst, pk_seg, tokens, labels, lp, seq_off, lp_off, scalars, per_token, eos, ref_lp=None):
    """The 12 columns of a packed step, each [pk_dst[-1]].  `scalars`: the five arrays of SCALAR_COLUMNS, [T_src] where the bit of
    `per_token` is set, [S] where it is not."""
    total = int(pk_dst[-1])
    out = {k: np.empty(total, dtype=np.int64) for k in I64_COLUMNS}
    out.update({k: np.empty(total, dtype=np.float32) for k in F32_COLUMNS})
    out["attention_mask"][:] = 1
    ref_src = lp if ref_lp is None else ref_lp
    filler = dict(rewards=0.0, advantages=0.0, group_tokens=1.0, num_labels=1.0, overflow=0.0)
    for j in range(len(pk_src)):
        b, e = int(pk_dst[j]), int(pk_dst[j + 1])
        n = e - b
        if n == 0:
            continue
        out["position_ids"][b:e] = np.arange(n)
        out["segment_ids"][b:e] = pk_seg[j]
        s = int(pk_src[j])
        if s < 0:
            out["input_ids"][b:e] = eos
            out["labels"][b:e] = -100
            out["ref_logprobs"][b:e] = 0.0
            out["old_logprobs"][b:e] = 0.0
            for k in SCALAR_COLUMNS:
                out[k][b:e] = filler[k]
            continue
        sb, lb, le = int(seq_off[s]), int(lp_off[s]), int(lp_off[s + 1])
        assert int(seq_off[s + 1]) - sb == n and 0 <= le - lb <= n
        out["input_ids"][b:e] = tokens[sb:sb + n]
        out["labels"][b:e] = labels[sb:sb + n]
        if pk_seg[j] > 0:
            out["labels"][b] = -100
        for name, src in (("old_logprobs", lp), ("ref_logprobs", ref_src)):
            out[name][b:e - (le - lb)] = 0.0
            out[name][e - (le - lb):e] = src[lb:le]
        for k, name in enumerate(SCALAR_COLUMNS):
            out[name][b:e] = scalars[k][sb:sb + n] if (per_token >> k) & 1 else scalars[k][s]
    return out


def pad_witness(row_src, padded_len, pad_left, tokens, labels, lp, seq_off, lp_off, scalars, per_token, ref_lp=None):
    """The 10 columns of a padded batch, each [len(row_src) * padded_len] (row-major)."""
    R = len(row_src)
    out = {k: np.zeros((R, padded_len), dtype=np.int64) for k in PAD_COLUMNS[:3]}
    out.update({k: np.zeros((R, padded_len), dtype=np.float32) for k in F32_COLUMNS})
    out["labels"][:] = -100
    ref_src = lp if ref_lp is None else ref_lp
    for r in range(R):
        s = int(row_src[r])
        sb, n, lb, le = int(seq_off[s]), int(seq_off[s + 1] - seq_off[s]), int(lp_off[s]), int(lp_off[s + 1])
        assert 0 <= n <= padded_len and 0 <= le - lb <= n
        b = padded_len - n if pad_left else 0
        e = b + n
        out["input_ids"][r, b:e] = tokens[sb:sb + n]
        out["labels"][r, b:e] = labels[sb:sb + n]
        out["attention_mask"][r, b:e] = 1
        out["old_logprobs"][r, e - (le - lb):e] = lp[lb:le]
        out["ref_logprobs"][r, e - (le - lb):e] = ref_src[lb:le]
        for k, name in enumerate(SCALAR_COLUMNS):
            out[name][r, b:e] = scalars[k][sb:sb + n] if (per_token >> k) & 1 else scalars[k][s]
    return {k: v.reshape(-1) for k, v in out.items()}


def oov_witness(tokens, valid, table_size, the_id):
    """(patched tokens int32, number of tokens patched).  `valid` may be None when table_size == 0."""
    t = np.asarray(tokens, dtype=np.int64)
    ok = (t >= 0) & (t < table_size)
    if table_size:
        ok[ok] = np.asarray(valid)[t[ok]] != 0
    return np.where(ok, t, the_id).astype(np.int32), int((~ok).sum())


# ---- cases ------------------------------------------------------------------------------------------------------------------------
def _f32(bits) -> np.ndarray:
    return np.asarray(bits, dtype=np.uint32).view(np.float32)


def _ragged(rng, lens, nlps, awkward=True):
    """Ragged source arrays with a distinct value in every slot, so that a value read from a wrong place shows: tokens 1000 + i,
    labels -100 on the first L - n_logprobs tokens of a sequence and 50 000 000 + i after them, log-probs / reference log-probs / the
    five per-token columns distinct positive-exponent bit patterns, the five per-sequence columns negative integers."""
    lens, nlps = np.asarray(lens, dtype=np.int64), np.asarray(nlps, dtype=np.int64)
    S = len(lens)
    seq_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    lp_off = np.concatenate([[0], np.cumsum(nlps)]).astype(np.int64)
    T, NL = int(seq_off[-1]), int(lp_off[-1])
    assert T < 2 ** 23 and S < 2 ** 16
    idx = np.arange(T, dtype=np.int64)
    tokens = (1000 + idx).astype(np.int32)
    within = idx - np.repeat(seq_off[:-1], lens)
    labelled = within >= np.repeat(lens - nlps, lens)
    labels = np.where(labelled, 50_000_000 + idx, -100).astype(np.int32)
    lp = _f32(0xBE000000 + np.arange(NL, dtype=np.int64))
    ref = _f32(0xBD000000 + np.arange(NL, dtype=np.int64))
    tok_scalars = np.stack([_f32(((0x40 + k) << 24) + idx) for k in range(5)])
    seq_scalars = np.stack([-(k * 65536 + np.arange(S) + 1.0) for k in range(5)]).astype(np.float32)
    if awkward and T > 64 and NL > 64 and S > 8:
        bits = _f32(AWKWARD_BITS)
        # ids and labels that change under a careless widening to int64 (labelled slots only: -100 keeps its meaning)
        lab_at = np.flatnonzero(labelled)
        labels[lab_at[rng.choice(len(lab_at), 3, replace=False)]] = (INT32_MIN, INT32_MAX, -1)
        tokens[rng.choice(T, 4, replace=False)] = (INT32_MIN, INT32_MAX, -1, 0)
        for arr in (lp, ref):
            arr[rng.choice(NL, 4 * len(bits), replace=False)] = np.tile(bits, 4)
            arr[:3] = bits[[0, 4, 1]]
        for k in range(5):  # disjoint sets: a per-token slot never holds what a per-sequence slot holds
            tok_scalars[k, rng.choice(T, 6, replace=False)] = np.tile(bits[[1, 2, 4]], 2)
            seq_scalars[k, rng.choice(S, 3, replace=False)] = bits[[0, 3, 5]]
    return dict(tokens=tokens, labels=labels, lp=lp, ref=ref, seq_off=seq_off, lp_off=lp_off, tok_scalars=tok_scalars,
                seq_scalars=seq_scalars)


def case_scalars(case, per_token):
    return [case["tok_scalars"][k] if (per_token >> k) & 1 else case["seq_scalars"][k] for k in range(5)]


class _PlanBuilder:
    """Plan entries in destination order: (length, n_logprobs or None for a filler, micro-batch)."""

    MODES = ("L", "0", "1", "L-1", "mid", "mid+1", "third")

    def __init__(self, zero_length=True):
        self.entries, self.pos, self.mb, self.cyc, self.mode, self.zero_length = [], 0, 0, 0, 0, zero_length
        self.pads = [0]

    def seq(self, L, nlp=None):
        if L == 0 and not self.zero_length:
            return
        if nlp is None:
            m = self.MODES[self.mode % len(self.MODES)]
            self.mode += 1
            nlp = {"L": L, "0": 0, "1": 1, "L-1": L - 1, "mid": L // 2, "mid+1": L // 2 + 1, "third": L // 3}[m]
        self.entries.append((L, min(max(nlp, 0), L), self.mb))
        self.pos += L

    def run(self, L, count):
        for _ in range(count):
            self.seq(L)

    def filler(self, n):
        """`n` filler tokens end the micro-batch (the planner appends the filler as a micro-batch's last slot)."""
        self.entries.append((n, None, self.mb))
        self.pos += n
        self.pads[-1] = n
        self.mb += 1
        self.pads.append(0)

    def fill_to(self, target):
        """CYCLE lengths in order up to `target`; a length that would pass it waits, and one sequence of the exact gap goes first."""
        assert target >= self.pos
        while self.pos < target:
            L = CYCLE[self.cyc % len(CYCLE)]
            if self.pos + L <= target:
                self.cyc += 1
                self.seq(L)
            else:
                self.seq(target - self.pos)

    def parity(self, p):
        if self.pos % 2 != p:
            self.seq(1)


def _edge_events(total):
    """(span start, kind, geometry) in token order: five events for each geometry, on span starts of that geometry (the aligned
    ones on starts that are not also unaligned starts).  Kinds: "at" a sequence starts on the span's first token, "before" / "after"
    one token either side, "zero" a zero-length sequence exactly there, "filler" a filler that spans it."""
    una = span_starts(total, False)
    ali = [p for p in span_starts(total, True) if p not in una]
    ev = [(p, k, False) for p, k in zip(una[1::2], ("at", "before", "after", "zero", "filler"))]
    ev += [(p, k, True) for p, k in zip(ali[0::2], ("after", "zero", "filler", "at", "before"))]
    assert len(ev) == 10
    return sorted(ev)


def _build_edges(zero_length):
    b = _PlanBuilder(zero_length)
    b.run(0, 3)                      # the first plan entries are zero-length
    b.run(1, 7)
    b.seq(9, 9)                      # token 0 labelled, carried by a seg == 0 sequence (the run above) ...
    extras = [lambda: b.run(1, 6), lambda: (b.parity(0), b.filler(1), b.seq(8, 8)), lambda: (b.parity(1), b.filler(1), b.run(0, 2), b.run(1, 6)),
              lambda: (b.parity(0), b.filler(2)), lambda: (b.parity(1), b.filler(2), b.seq(5, 5)), lambda: (b.run(2, 6), b.run(3, 6)),
              lambda: (b.parity(0), b.filler(3)), lambda: (b.parity(1), b.filler(3), b.seq(0), b.seq(4, 4)), lambda: (b.seq(7, 7), b.run(0, 4), b.seq(7, 7)),
              lambda: b.run(1, 9)]
    for (p, kind, aligned), extra in zip(_edge_events(EDGE_TOTAL), extras):
        if kind in ("at", "zero"):
            b.fill_to(p)
            if kind == "zero":
                b.run(0, 1 if aligned else 2)
            b.seq(6)
        elif kind == "before":
            b.fill_to(p - 1)
            b.seq(6)
        elif kind == "after":
            b.fill_to(p - 2)
            b.seq(3)                 # ends one token past the span start
            b.seq(6)
        else:
            b.fill_to(p - 1)
            b.filler(2 if aligned else 3)
            b.run(0, 2)              # zero-length sequences directly after a filler
            b.seq(6, 6)              # ... and here by the first sequence of a micro-batch
        extra()
    b.fill_to(EDGE_TOTAL - 9)
    b.run(1, 6)
    b.filler(3)                      # the last tokens, the odd one included, are a filler's
    b.run(0, 2)                      # the last plan entries are zero-length (a micro-batch of their own)
    assert b.pos == EDGE_TOTAL
    return b


@functools.lru_cache(maxsize=None)
def pack_case(name):
    """dict: the ragged arrays of `_ragged`, the plan pk_src / pk_dst / pk_seg, `micro_batches` (source indices) and `pads` it comes
    from, eos.  "edges" / "edges_nz" (the same without zero-length sequences) / "long"."""
    if name == "long":
        return _long_case()
    rng = np.random.default_rng(53)
    b = _build_edges(zero_length=(name == "edges"))
    real = [i for i, e in enumerate(b.entries) if e[1] is not None]
    spare = [(5, 2), (0, 0), (17, 17)]              # sources no plan entry uses
    perm = rng.permutation(len(real) + len(spare))  # plan order is not source order
    S = len(perm)
    lens, nlps = np.zeros(S, dtype=np.int64), np.zeros(S, dtype=np.int64)
    pk_src, pk_seg, pk_len, mbs = [], [], [], [[] for _ in b.pads]
    r, seg, mb_now = 0, 0, 0
    for L, nlp, mb in b.entries:
        if mb != mb_now:
            mb_now, seg = mb, 0
        if nlp is None:
            pk_src.append(-1)
        else:
            s = int(perm[r])
            r += 1
            lens[s], nlps[s] = L, nlp
            pk_src.append(s)
            mbs[mb].append(s)
        pk_seg.append(seg)
        pk_len.append(L)
        seg += 1
    for (L, nlp), s in zip(spare, perm[r:]):
        lens[s], nlps[s] = L, nlp
    while mbs and not mbs[-1] and not b.pads[len(mbs) - 1]:  # reduced case: the trailing micro-batch of zero-length sequences is gone
        mbs.pop()
    case = _ragged(rng, lens, nlps)
    case.update(pk_src=np.asarray(pk_src, dtype=np.int32), pk_seg=np.asarray(pk_seg, dtype=np.int32),
                pk_dst=np.concatenate([[0], np.cumsum(pk_len)]).astype(np.int64), micro_batches=mbs, pads=b.pads[:len(mbs)], eos=EOS)
    return case


def _long_case():
    rng = np.random.default_rng(59)
    lens, nlps, pk_src, pk_seg, pk_len = [], [], [], [], []
    pos = seg = 0
    draws = rng.integers(1, 701, 20000).tolist()
    frac = rng.random(20000).tolist()
    for i, L in enumerate(draws):
        if i % 37 == 36:  # an occasional filler of 1 .. 3 tokens ends a micro-batch
            n = min(1 + i % 3, LONG_TOTAL - pos)
            pk_src.append(-1)
            pk_len.append(n)
            pk_seg.append(seg)
            seg = 0
        else:
            L = min(L if i % 11 else 1 + i % 3, LONG_TOTAL - pos)  # every eleventh sequence is 1 .. 3 tokens long
            n = L
            pk_src.append(len(lens))
            pk_len.append(L)
            pk_seg.append(seg)
            lens.append(L)
            nlps.append((0, L, int(frac[i] * (L + 1)))[i % 3])
            seg += 1
        pos += n
        if pos == LONG_TOTAL:
            break
    assert pos == LONG_TOTAL
    case = _ragged(rng, lens, nlps)
    case.update(pk_src=np.asarray(pk_src, dtype=np.int32), pk_seg=np.asarray(pk_seg, dtype=np.int32),
                pk_dst=np.concatenate([[0], np.cumsum(pk_len)]).astype(np.int64), micro_batches=None, pads=None, eos=EOS)
    return case


PAD_LEN = 48


@functools.lru_cache(maxsize=None)
def pad_case(name):
    """dict: the ragged arrays, row_src, padded_len.  "edges": rows of 0, 1, padded_len - 1 and padded_len tokens and two in between,
    `row_src` permuted with a repeat, log-prob counts 0, L and in between.  "stride": 70 x 16 000 = 1 120 000 entries, past the
    1 048 576 that 4096 workgroups of 256 cover in one trip."""
    if name == "edges":
        rng = np.random.default_rng(61)
        lens = [0, 1, PAD_LEN - 1, PAD_LEN, 5, 17, PAD_LEN, 30]
        nlps = [0, 1, 0, PAD_LEN, 2, 17, 11, 29]
        case = _ragged(rng, lens, nlps)
        case.update(row_src=np.asarray([3, 0, 7, 2, 1, 3, 5, 4, 6, 0, 2], dtype=np.int32), padded_len=PAD_LEN)
        return case
    rng = np.random.default_rng(67)
    padded = 16000
    lens = rng.integers(0, padded + 1, 40)
    lens[:4] = (padded, 0, padded - 1, 1)
    nlps = (lens * rng.random(40)).astype(np.int64)
    nlps[:6] = (padded, 0, 0, 1, lens[4], 0)
    case = _ragged(rng, lens, nlps)
    rows = np.concatenate([rng.permutation(40), rng.integers(0, 40, 30)]).astype(np.int32)
    case.update(row_src=rows, padded_len=padded)
    assert len(rows) * padded > STRIDE_ITEMS
    return case


@functools.lru_cache(maxsize=None)
def oov_case(name):
    """dict: tokens int32 [n], valid uint8 [table_size] or None, table_size, the_id.  "edges" (the last table entry and the_id valid),
    "the_invalid" (both invalid: what was patched is found invalid again), "empty" (table_size 0, no table: everything is patched),
    "stride" (1 200 000 tokens, about a tenth invalid)."""
    if name == "stride":
        rng = np.random.default_rng(71)
        size, n = 5000, 1_200_000
        valid = (rng.random(size) >= 0.1).astype(np.uint8)
        the_id = int(np.flatnonzero(valid)[7])
        tokens = rng.integers(0, size, n).astype(np.int32)
        tokens[rng.choice(n, 64, replace=False)] = np.tile(np.asarray([-1, INT32_MIN, size, INT32_MAX], dtype=np.int32), 16)
        assert n > STRIDE_ITEMS
        return dict(tokens=tokens, valid=valid, table_size=size, the_id=the_id)
    rng = np.random.default_rng(73)
    size, n, the_id = 50, 777, 11
    valid = (rng.random(size) >= 0.3).astype(np.uint8)
    valid[[0, the_id, size - 1]] = 1
    valid[[1, size - 2]] = 0
    tokens = rng.integers(-5, size + 6, n).astype(np.int32)
    special = np.asarray([-1, INT32_MIN, 0, size - 1, size, INT32_MAX, the_id, 1, size - 2], dtype=np.int32)
    tokens[:len(special)] = special
    tokens[-len(special):] = special[::-1]
    if name == "the_invalid":
        valid[[the_id, size - 1]] = 0
    elif name == "empty":
        return dict(tokens=tokens, valid=None, table_size=0, the_id=the_id)
    else:
        assert name == "edges"
    return dict(tokens=tokens, valid=valid, table_size=size, the_id=the_id)


# ---- checker ----------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Mismatch:
    column: str
    token: int
    entry: int | None = None   # plan entry (packed sequence) that owns the token
    segment: int | None = None
    region: str | None = None
    got: object = None
    want: object = None

    def __str__(self):
        where = "" if self.entry is None else f" (plan entry {self.entry}, segment {self.segment}, {self.region})"
        return f"{self.column}[{self.token}]{where}: got {self.got!r}, want {self.want!r}"


def _bits(a):
    a = np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def token_region(t, pk_src, pk_dst, tpl):
    """(plan entry, region) of token t under `tpl` tokens per lane: "filler" a filler's token; "tail" the last, partial lane group;
    "fast" the lane group lies inside one sequence; "straddling" it holds a sequence boundary."""
    j = int(np.searchsorted(pk_dst, t, side="right")) - 1
    t0 = t - t % tpl
    if pk_src[j] < 0:
        return j, "filler"
    if t0 + tpl > int(pk_dst[-1]):
        return j, "tail"
    return j, ("fast" if t0 >= pk_dst[j] and t0 + tpl <= pk_dst[j + 1] else "straddling") + (" pair" if tpl == 2 else " quad")


def first_mismatch(got, want, plan=None, tpl=2):
    """The mismatch at the smallest token index over all columns of `want` (ties: column order), or None.  Every entry of every column
    is compared, fp32 columns as uint32.  `plan` = (pk_src, pk_dst, pk_seg) names the token's plan entry, segment and region."""
    best = None
    for name, w in want.items():
        g = np.asarray(got[name])
        assert g.shape == w.shape and g.dtype == w.dtype, f"{name}: got {g.dtype}{g.shape}, want {w.dtype}{w.shape}"
        bad = np.flatnonzero(_bits(g) != _bits(w))
        if len(bad) and (best is None or bad[0] < best.token):
            t = int(bad[0])
            best = Mismatch(name, t, got=g[t], want=w[t])
    if best is not None and plan is not None:
        pk_src, pk_dst, pk_seg = plan
        best.entry, best.region = token_region(best.token, pk_src, pk_dst, tpl)
        best.segment = int(pk_seg[best.entry])
    return best


def check_columns(got, want, plan=None, tpl=2):
    bad = first_mismatch(got, want, plan, tpl)
    assert bad is None, str(bad)


# ---- bounds: nothing a launch is handed may point outside its buffer --------------------------------------------------------------
def check_ragged_bounds(case):
    T, NL, S = len(case["tokens"]), len(case["lp"]), len(case["seq_off"]) - 1
    assert len(case["labels"]) == T and len(case["ref"]) == NL and case["tok_scalars"].shape == (5, T) and case["seq_scalars"].shape == (5, S)
    for off, n in ((case["seq_off"], T), (case["lp_off"], NL)):
        assert off.dtype == np.int64 and len(off) == S + 1 and off[0] == 0 and off[-1] == n and (np.diff(off) >= 0).all()
    assert (np.diff(case["lp_off"]) <= np.diff(case["seq_off"])).all(), "more log-probs than tokens in a sequence"
    assert all(case[k].dtype == np.int32 for k in ("tokens", "labels")) and all(case[k].dtype == np.float32 for k in ("lp", "ref", "tok_scalars", "seq_scalars"))


def check_pack_bounds(case):
    """Every source index, log-prob range and destination range of a pack case lies inside its buffer."""
    check_ragged_bounds(case)
    src, dst, seg = case["pk_src"], case["pk_dst"], case["pk_seg"]
    S, m = len(case["seq_off"]) - 1, len(src)
    assert src.dtype == np.int32 and seg.dtype == np.int32 and dst.dtype == np.int64 and len(dst) == m + 1 and len(seg) == m
    assert dst[0] == 0 and (np.diff(dst) >= 0).all() and dst[-1] > 0 and (seg >= 0).all()
    assert (src >= -1).all() and (src < S).all()
    real = src >= 0
    assert np.array_equal(np.diff(dst)[real], np.diff(case["seq_off"])[src[real]]), "a destination range is not its source's length"


def check_pad_bounds(case):
    check_ragged_bounds(case)
    rows = case["row_src"]
    assert rows.dtype == np.int32 and (rows >= 0).all() and (rows < len(case["seq_off"]) - 1).all()
    assert (np.diff(case["seq_off"]) <= case["padded_len"]).all()


def check_oov_bounds(case):
    assert case["tokens"].dtype == np.int32 and 0 <= case["the_id"]
    assert (case["valid"] is None and case["table_size"] == 0) or (case["valid"].dtype == np.uint8 and len(case["valid"]) == case["table_size"])
