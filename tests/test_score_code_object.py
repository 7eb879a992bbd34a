"""The gfx950 code objects of the score form of the SDDMM (sparta_vbs_sddmm_block_ssq), checked without a GPU (metadata fields only, through
_kernel_metadata of tests/test_code_object.py).

The score kernels are the bodies of the live SDDMM kernels with a reduction where the store was: shuffles, no LDS of their own, nothing in scratch.  The
finish kernel is register-only, as the kernels of k_prune.hip.  None of the new names holds a substring the other code-object tests count kernels by."""
from test_code_object import _kernel_metadata


def test_score_kernels(tmp_path):
    kernels = _kernel_metadata(tmp_path)
    score = {n: m for n, m in kernels.items() if "vbs_sdscore_" in n}
    product = {n: m for n, m in score.items() if "vbs_sdscore_finish_kernel" not in n}
    finish = {n: m for n, m in score.items() if "vbs_sdscore_finish_kernel" in n}
    live = {n: m for n, m in kernels.items() if "vbs_sdlive_" in n}
    assert len(product) == 5 and len(finish) == 1 and len(live) == 5, sorted(score)          # fp32 + <BF16, VEC> x 4, and the finish kernel
    assert sum("vbs_sdscore_f32_kernel" in n for n in product) == 1 and sum("vbs_sdscore_h16_kernelILb" in n for n in product) == 4
    for name, m in score.items():
        assert not any(s in name for s in ("vbs_sddmm_", "vbs_sdlive_", "vbs_live_", "vbs_prune_")), name
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (name, m)
    for name, m in finish.items():
        assert m["group_segment_fixed_size"] == 0, (name, m)
    for name, m in product.items():
        form = name.split("vbs_sdscore_")[1].split("NS_")[0]          # "f32_kernelE" or "h16_kernelILb.ELb.EEEv": the kernel and its template arguments
        cands = [n for n in live if ("vbs_sdlive_" + form) in n]
        assert len(cands) == 1, (name, form, sorted(live))
        assert m["group_segment_fixed_size"] <= live[cands[0]]["group_segment_fixed_size"], (name, m, live[cands[0]])
