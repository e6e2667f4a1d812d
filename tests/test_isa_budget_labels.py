"""Build-time guard for the label-map kernel (csrc/det_post_labels.hpp), in the manner of tests/test_isa_budget_sized.py: both
instantiations of k_detpost_labels keep everything in registers -- no scratch, no spill -- stay within the 128 VGPRs that leave
four wavefronts per SIMD, and hold the static LDS the header states (no GPU needed)."""
import shutil
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tools"))


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_the_label_kernel_has_no_scratch_and_no_spill():
    import isa_stats
    st = isa_stats.collect()
    labels = {k: v for k, v in st.items() if "k_detpost_labels" in k}
    assert len(labels) == 2                                     # fp16 and fp32 prototypes
    for k, v in labels.items():
        assert v["scratch"] == 0 and v["spill"] == 0, (k, v)
        assert v["vgpr"] <= 128 and v["agpr"] == 0 and v["wg"] == 256, (k, v)
        assert v["lds"] == 256 * 16 + 2048 * 4 + 8, (k, v)      # the staged boxes, the patch, the two flags
        assert v["mfma"] == 0 and v["lds_op"] > 0, (k, v)
