"""The fused body kernels are memory-bound streaming kernels: cross-compiled for gfx950, none of them may spill (scratch 0) or
need more than 128 VGPRs (four waves per SIMD stay resident)."""

import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "scripts"))

from check_mfma_hazards import compile_to_asm, kernel_resources  # noqa: E402
from pipelinerl_amd.fused_body import rms_norm  # noqa: E402,F401  (the feature these kernels belong to)

KERNELS = ("rmsnorm_fwd_kernel", "rmsnorm_bwd_kernel", "rmsnorm_dw_fold_kernel", "swiglu_fwd_kernel", "swiglu_bwd_kernel")


def test_no_scratch_and_at_most_128_vgprs():
    res = kernel_resources(compile_to_asm(("prl_body.hip",)))
    for k in KERNELS:
        assert any(k in name for name in res), f"{k} is not in the listing"
    for name, r in res.items():
        print(f"[body] {name}: {r}")
        assert r["scratch"] == 0, (name, r)
        assert r["vgpr"] <= 128, (name, r)
        assert r["lds"] % 16 == 0, (name, r)
