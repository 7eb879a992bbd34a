"""The compiled gfx950 code object of the kernel of k_repattern.hip (sparta_vbs_move_blocks), checked without a GPU: metadata fields only.  A bandwidth-bound
copy whose few staged vectors must stay in registers: no private (scratch) segment, no VGPR spill, no LDS (one wave per block: nothing crosses a wave), and
few enough registers for eight waves per SIMD.  Its name matches none of the patterns other tests count kernels by."""
from test_code_object import _kernel_metadata

# what the tests of the other kernel families filter names on
FOREIGN = ("vbs_prune_", "vbs_adam_", "vbs_sgd_", "vbs_update_", "stream_kernel", "direct_kernel", "sddmm", "gradctl", "vbs_epilogue_", "vbs_live_",
           "live_blocks_kernel", "blocks_kernel", "vbs_lvstep_", "vbs_sgdlive_", "vbs_adamlive_", "vbs_sdscore_", "vbs_sdlive_", "vbs_spmm_", "colres_kernel",
           "vbs_union_", "packed_kernel")


def test_the_move_kernel_keeps_its_state_in_registers(tmp_path):
    kernels = _kernel_metadata(tmp_path)
    rp = {n: m for n, m in kernels.items() if "vbs_repat_" in n}
    assert len(rp) == 1 and "vbs_repat_move_kernel" in next(iter(rp)), sorted(rp)
    for name, m in rp.items():
        assert m["private_segment_fixed_size"] == 0, (name, m)
        assert m["vgpr_spill_count"] == 0, (name, m)
        assert m["group_segment_fixed_size"] == 0, (name, m)
        assert m["vgpr_count"] <= 64, (name, m)                           # 512 / 64: eight waves per SIMD
        assert not any(p in name for p in FOREIGN), name
