"""The slice-form attention kernels cross-compiled for gfx950: every one is in the listing for both head sizes, none spills
(scratch 0), and their LDS is a multiple of 16 bytes within the 160 KiB of a CU."""

import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "scripts"))

from check_mfma_hazards import compile_to_asm, kernel_resources  # noqa: E402
from pipelinerl_amd.fused_attention import varlen_attention_slice  # noqa: E402,F401  (the feature these kernels belong to)

BY_HEAD_SIZE = ("attn_slice_fwd_kernel", "attn_slice_delta_kernel", "attn_slice_dkv_kernel", "attn_slice_dq_kernel")
SQUARE = ("attn_fwd_kernel", "attn_dkv_kernel", "attn_dq_kernel", "attn_delta_kernel", "attn_segments_kernel")


def test_no_scratch_and_lds_within_a_cu():
    res = kernel_resources(compile_to_asm(("prl_attention_sp.hip",)))
    for k in BY_HEAD_SIZE:  # both head sizes are built
        assert sum(k in name for name in res) == 2, (k, list(res))
    assert sum("attn_slice_fold_kernel" in name for name in res) == 2, list(res)  # 16-byte pieces, and the form for any length
    for name, r in res.items():
        print(f"[attention sp] {name}: {r}")
        assert not any(k in name for k in SQUARE), f"{name} would be counted among the square kernels"
        assert r["scratch"] == 0, (name, r)
        assert r["lds"] <= 160 * 1024, (name, r)
        assert r["lds"] % 16 == 0, (name, r)
    assert max(r["lds"] for r in res.values()) > 0
