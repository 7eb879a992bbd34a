"""The gfx950 code objects of the live-block set, checked without a GPU (metadata fields only, through _kernel_metadata of tests/test_code_object.py).

The compaction kernels of k_live.hip are register-only by design (ballot + prefix count: no LDS, nothing in scratch).  The live forms of the SDDMM kernels
must not cost their unmasked siblings anything and must themselves stay in the same occupancy class: same LDS, no scratch, no spill, and a register count
that allows the same number of waves per SIMD (512 registers per lane and SIMD, allocated in units of 8, at most 8 waves)."""
from test_code_object import _kernel_metadata


def _waves(vgprs):
    return min(8, 512 // (max((vgprs + 7) // 8, 1) * 8))


def test_compaction_kernels_use_registers_only(tmp_path):
    kernels = _kernel_metadata(tmp_path)
    ks = {n: m for n, m in kernels.items() if "vbs_live_" in n}
    assert len(ks) == 2 and any("vbs_live_groups_kernel" in n for n in ks) and any("vbs_live_columns_kernel" in n for n in ks), sorted(ks)
    for name, m in ks.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["group_segment_fixed_size"] == 0, (name, m)


def test_live_sddmm_kernels_match_their_siblings(tmp_path):
    """vbs_sdlive_f32_kernel / vbs_sdlive_h16_kernel<BF16, VEC> next to vbs_sddmm_f32_kernel / vbs_sddmm_h16_kernel<BF16, VEC>"""
    kernels = _kernel_metadata(tmp_path)
    live = {n: m for n, m in kernels.items() if "vbs_sdlive_" in n}
    plain = {n: m for n, m in kernels.items() if "vbs_sddmm_" in n}
    assert len(live) == 5 and len(plain) == 5, (sorted(live), sorted(plain))                  # fp32 + <BF16, VEC> x 4, each form
    for name, m in live.items():
        form = name.split("vbs_sdlive_")[1].split("NS_")[0]           # "f32_kernelE" or "h16_kernelILb.ELb.EEEv": the kernel and its template arguments
        cands = [n for n in plain if ("vbs_sddmm_" + form) in n]
        assert len(cands) == 1, (name, form, sorted(plain))
        s = plain[cands[0]]
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (name, m)
        assert s["private_segment_fixed_size"] == 0 and s["vgpr_spill_count"] == 0, (cands[0], s)
        assert m["group_segment_fixed_size"] == s["group_segment_fixed_size"], (name, m, s)
        assert _waves(m["vgpr_count"]) == _waves(s["vgpr_count"]), (name, m["vgpr_count"], s["vgpr_count"])


def test_unmasked_backward_kernels_keep_their_names(tmp_path):
    kernels = _kernel_metadata(tmp_path)
    assert sum("vbs_sddmm_f32_kernel" in n for n in kernels) == 1
    assert sum("vbs_sddmm_h16_kernelILb" in n for n in kernels) == 4
    assert sum("vbs_spmm_t_f32_kernel" in n for n in kernels) == 1
    assert sum("vbs_spmm_t_h16_kernelILb" in n for n in kernels) == 2
