"""Build-time guard for the table forms of the two fused stems (per-stream frame sizes): the budget of their scalar twins in
tests/test_isa_budget.py, and names that the substring searches of that file do not pick up (no GPU needed)."""
import shutil
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tools"))


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")
def test_table_form_stems_keep_the_budget_of_their_scalar_twins():
    import isa_stats
    st = isa_stats.collect()
    find = lambda sub: {k: v for k, v in st.items() if sub in k}
    stem = find("k_stem_sized_fusedE")
    assert len(stem) == 1
    for k, v in stem.items():
        assert v["vgpr"] <= 128 and v["scratch"] == 0 and v["mfma"] == 63, (k, v)
    stem_hp = find("k_stem_sized_fused_hp")
    assert len(stem_hp) == 1
    for k, v in stem_hp.items():
        assert v["vgpr"] <= 128 and v["scratch"] <= 32 and v["mfma"] == 126, (k, v)
    # the frame-size lookup is scalar: no vector memory instruction more than the scalar form has
    for sized, scalar in (("k_stem_sized_fusedE", "k_stem_resize_fusedE"), ("k_stem_sized_fused_hp", "k_stem_resize_fused_hp"),
                          ("k_crop_resize_rgbx_sizedE", "k_crop_resize_rgbxE"), ("k_crop_resize_rgbx_hl_sized", "k_crop_resize_rgbx_hlE"),
                          ("k_crop_resize_sizedIfE", "k_crop_resizeIfE")):
        (a,), (b,) = find(sized).values(), find(scalar).values()
        assert a["vmem"] == b["vmem"] and a["vgpr"] == b["vgpr"], (sized, a, b)
    # the searches of tests/test_isa_budget.py see what they saw
    assert len(find("k_stem_resize_fusedE")) == 1 and len(find("k_stem_resize_fused_hp")) == 1 and len(find("k_osblock_hp")) == 6
