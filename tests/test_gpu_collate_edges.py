"""K6 `pack_collate_kernel`, K7 `pad_collate_kernel` and `patch_oov_kernel` of csrc/prl_pack.hip, through the C ABI
(`prl_pack_collate`, `prl_pad_collate`, `prl_patch_oov`), against the plain witnesses of tests/collate_checks.py: every entry of every
column, exactly (fp32 columns as uint32), with canary-filled guards around every output column.

What the cases reach that workload-shaped parity did not (tests/test_collate_checks_host.py asserts each is present):

  pack "edges"   12 001 tokens in 10 micro-batches: runs of zero-length and of 1-, 2- and 3-token sequences (first plan entries, last
                 plan entries, directly after a filler); a sequence start on a workgroup span's first token and one token either side,
                 a zero-length sequence exactly there and a filler across it, for the two-tokens-per-lane and the four-tokens-per-lane
                 geometry each; fillers of 1, 2, 3 tokens on both parities and as the odd last token; the left-padding edge of the
                 log-probs on both parities of the sequence start; each `per_token_columns` bit alone; `ref_logprobs == NULL`.
                 Outputs one element off 16-byte alignment launch `pack_collate_kernel<false, false, 4>`, which no test reached.
  pack "long"    4 400 001 tokens: three lane iterations at two tokens per lane, two at four, on the capped grid of 4096 workgroups.
  pad, oov       rows of 0 / 1 / padded_len - 1 / padded_len tokens on both sides, a repeated source row, 1 120 000 entries and
                 1 200 000 tokens (past one trip of the grid-stride loops), ids at both ends of the table and of int32, the_id itself
                 invalid, no table at all.

Defects found: none so far.  A line-by-line host replay of K6's span split, lane walk and both branches equals the witness on
"edges" for both geometries; these tests have not yet been run on an MI355X, so wall times and a verdict from the device are open."""

import functools

import numpy as np
import pytest
import torch

import collate_checks as cc

GUARD = 64                      # canary elements after (and `lead` before) every output column
CANARY32 = 0x7B7B7B7B           # every 4-byte word of a fresh output buffer


def _dev(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _outputs(names, total, dev, aligned):
    """name -> (whole buffer, view handed to the kernel).  Unaligned: every view starts one element into its buffer."""
    lead = 0 if aligned else 1
    out = {}
    for name in names:
        dt = torch.int64 if name in cc.I64_COLUMNS else torch.float32
        buf = torch.empty(lead + total + GUARD, dtype=dt, device=dev)
        buf.view(torch.int32).fill_(CANARY32)
        view = buf[lead:lead + total]
        assert (view.data_ptr() % 16 == 0) == aligned and view.data_ptr() % buf.element_size() == 0, name
        out[name] = (buf, view)
    return out


def _guards_intact(out, total):
    for name, (buf, view) in out.items():
        lead = view.storage_offset()
        outside = torch.cat([buf[:lead], buf[lead + total:]]).view(torch.int32)
        assert outside.numel() >= GUARD and bool((outside == CANARY32).all()), f"{name}: a guard element was written"


def _as_int(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _upload_ragged(case, per_token, with_ref, dev):
    d = {k: _dev(case[k], dev) for k in ("tokens", "labels", "lp", "seq_off", "lp_off")}
    d["ref"] = _dev(case["ref"], dev) if with_ref else None
    d["scalars"] = [_dev(a, dev) for a in cc.case_scalars(case, per_token)]
    return d


@pytest.fixture(scope="module")
def pack_seen():
    """(per_token, with_ref) -> {aligned: columns}: the two launch forms of K6 must write the same bytes."""
    return {}


def run_pack(lib, dev, case, per_token, with_ref, aligned):
    from pipelinerl_amd import _lib

    cc.check_pack_bounds(case)
    p = _lib.ptr
    total, m = int(case["pk_dst"][-1]), len(case["pk_src"])
    d = _upload_ragged(case, per_token, with_ref, dev)
    plan = [_dev(case[k], dev) for k in ("pk_src", "pk_dst", "pk_seg")]
    out = _outputs(cc.PACK_COLUMNS, total, dev, aligned)
    with torch.cuda.device(dev):
        _lib.check(lib.prl_pack_collate(m, total, *[p(x) for x in plan], p(d["tokens"]), p(d["labels"]), p(d["lp"]), p(d["ref"]), p(d["seq_off"]),
                                        p(d["lp_off"]), *[p(x) for x in d["scalars"]], per_token, case["eos"],
                                        *[p(out[k][1]) for k in cc.PACK_COLUMNS], _lib.current_stream_ptr(dev)))
    torch.cuda.synchronize(dev)
    return out


def _pack_want(case, per_token, with_ref):
    return cc.pack_witness(case["pk_src"], case["pk_dst"], case["pk_seg"], case["tokens"], case["labels"], case["lp"], case["seq_off"],
                           case["lp_off"], cc.case_scalars(case, per_token), per_token, case["eos"], case["ref"] if with_ref else None)


@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("with_ref", [True, False], ids=["ref", "noref"])
@pytest.mark.parametrize("per_token", [0, 1, 2, 4, 8, 16, 31])
def test_pack_edges(libprl, cuda_device, pack_seen, per_token, with_ref, aligned):
    case = cc.pack_case("edges")
    total = int(case["pk_dst"][-1])
    out = run_pack(libprl, cuda_device, case, per_token, with_ref, aligned)
    got = {k: v.cpu().numpy() for k, (_, v) in out.items()}
    cc.check_columns(got, _pack_want(case, per_token, with_ref), (case["pk_src"], case["pk_dst"], case["pk_seg"]), cc.pack_geometry(total, aligned)[0])
    _guards_intact(out, total)
    seen = pack_seen.setdefault((per_token, with_ref), {})
    seen[aligned] = got
    if len(seen) == 2:
        cc.check_columns(seen[False], seen[True], (case["pk_src"], case["pk_dst"], case["pk_seg"]), 4)


@functools.lru_cache(maxsize=1)
def _long_want(per_token):
    return _pack_want(cc.pack_case("long"), per_token, True)


@pytest.mark.gpu
@pytest.mark.parametrize("per_token,aligned", [(0, True), (0, False), (31, True), (31, False)], ids=["pt0-aligned", "pt0-unaligned", "pt31-aligned", "pt31-unaligned"])
def test_pack_long(libprl, cuda_device, per_token, aligned):
    case = cc.pack_case("long")
    total = int(case["pk_dst"][-1])
    tpl, n_blocks, per_block = cc.pack_geometry(total, aligned)
    iters = cc.lane_iterations(total, aligned)
    print(f"[k6 long] {total} tokens, {tpl} per lane: {n_blocks} workgroups x {per_block} lane groups, {iters} lane iterations")
    assert n_blocks == cc.MAX_BLOCKS and iters == (3 if aligned else 2)
    want = _long_want(per_token)
    out = run_pack(libprl, cuda_device, case, per_token, True, aligned)
    for k in cc.PACK_COLUMNS:  # whole columns, on the device; the host checker only names a mismatch
        if not torch.equal(_as_int(out[k][1]), _as_int(_dev(want[k], cuda_device))):
            cc.check_columns({k: out[k][1].cpu().numpy()}, {k: want[k]}, (case["pk_src"], case["pk_dst"], case["pk_seg"]), tpl)
            raise AssertionError(f"{k}: the device and the host comparison disagree")
    _guards_intact(out, total)


def run_pad(lib, dev, case, per_token, with_ref, pad_left):
    from pipelinerl_amd import _lib

    cc.check_pad_bounds(case)
    p = _lib.ptr
    R, P = len(case["row_src"]), int(case["padded_len"])
    d = _upload_ragged(case, per_token, with_ref, dev)
    rows = _dev(case["row_src"], dev)
    out = _outputs(cc.PAD_COLUMNS, R * P, dev, aligned=True)
    with torch.cuda.device(dev):
        _lib.check(lib.prl_pad_collate(R, P, int(pad_left), p(rows), p(d["tokens"]), p(d["labels"]), p(d["lp"]), p(d["ref"]), p(d["seq_off"]), p(d["lp_off"]),
                                       *[p(x) for x in d["scalars"]], per_token, *[p(out[k][1]) for k in cc.PAD_COLUMNS], _lib.current_stream_ptr(dev)))
    torch.cuda.synchronize(dev)
    want = cc.pad_witness(case["row_src"], P, pad_left, case["tokens"], case["labels"], case["lp"], case["seq_off"], case["lp_off"],
                          cc.case_scalars(case, per_token), per_token, case["ref"] if with_ref else None)
    cc.check_columns({k: v.cpu().numpy() for k, (_, v) in out.items()}, want)
    _guards_intact(out, R * P)


@pytest.mark.gpu
@pytest.mark.parametrize("with_ref", [True, False], ids=["ref", "noref"])
@pytest.mark.parametrize("per_token", [0, 1, 2, 4, 8, 16, 31])
@pytest.mark.parametrize("side", ["right", "left"])
def test_pad_edges(libprl, cuda_device, side, per_token, with_ref):
    run_pad(libprl, cuda_device, cc.pad_case("edges"), per_token, with_ref, side == "left")


@pytest.mark.gpu
@pytest.mark.parametrize("per_token", [0, 31])
@pytest.mark.parametrize("side", ["right", "left"])
def test_pad_stride(libprl, cuda_device, side, per_token):
    run_pad(libprl, cuda_device, cc.pad_case("stride"), per_token, True, side == "left")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["edges", "the_invalid", "empty", "stride"])
def test_patch_oov(libprl, cuda_device, name):
    from pipelinerl_amd import _lib

    case = cc.oov_case(name)
    cc.check_oov_bounds(case)
    dev, n = cuda_device, len(case["tokens"])
    want, n_bad = cc.oov_witness(case["tokens"], case["valid"], case["table_size"], case["the_id"])
    again = cc.oov_witness(want, case["valid"], case["table_size"], case["the_id"])[1]
    the_valid = case["table_size"] > 0 and bool(case["valid"][case["the_id"]])
    assert again == (0 if the_valid else n_bad) and n_bad > 0 and (name != "empty" or n_bad == n)

    def buffer():
        buf = torch.full((n + GUARD,), CANARY32, dtype=torch.int32, device=dev)
        buf[:n] = _dev(case["tokens"], dev)
        return buf
    buf, buf_nocount = buffer(), buffer()
    valid = _dev(case["valid"], dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        stream = _lib.current_stream_ptr(dev)
        call = lambda b, c: _lib.check(libprl.prl_patch_oov(n, _lib.ptr(b), _lib.ptr(valid), case["table_size"], case["the_id"], _lib.ptr(c), stream))  # noqa: E731
        call(buf, count)
        first, first_count = buf.clone(), count.clone()  # stream-ordered copies: read after the one synchronize below
        call(buf, count)                                  # the counter accumulates
        call(buf_nocount, None)                           # patched == NULL is accepted
    torch.cuda.synchronize(dev)
    for label, b in (("first call", first), ("second call", buf), ("without a counter", buf_nocount)):
        cc.check_columns({label: b[:n].cpu().numpy()}, {label: want})
        assert bool((b[n:] == CANARY32).all()), f"{label}: a guard element was written"
    assert int(first_count) == n_bad and int(count) == n_bad + again
