"""The attention kernels cross-compiled for gfx950: every one is in the listing, none spills (scratch 0), and their LDS is a
multiple of 16 bytes within the 160 KiB of a CU."""

import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "scripts"))

from check_mfma_hazards import compile_to_asm, kernel_resources  # noqa: E402
from pipelinerl_amd.fused_attention import varlen_attention  # noqa: E402,F401  (the feature these kernels belong to)

KERNELS = ("attn_segments_kernel", "attn_fwd_kernel", "attn_delta_kernel", "attn_dkv_kernel", "attn_dq_kernel")


def test_no_scratch_and_lds_within_a_cu():
    res = kernel_resources(compile_to_asm(("prl_attention.hip",)))
    for k in KERNELS:
        assert any(k in name for name in res), f"{k} is not in the listing"
    for k in ("attn_fwd_kernel", "attn_dkv_kernel", "attn_dq_kernel"):  # both head sizes are built
        assert sum(k in name for name in res) == 2, (k, list(res))
    for name, r in res.items():
        print(f"[attention] {name}: {r}")
        assert r["scratch"] == 0, (name, r)
        assert r["lds"] <= 160 * 1024, (name, r)
        assert r["lds"] % 16 == 0, (name, r)
