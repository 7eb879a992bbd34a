"""The compiled gfx950 code object of the two kernels of k_prune.hip (sparta_vbs_block_ssq / sparta_vbs_mask_blocks), checked without a GPU: metadata
fields only.  Both are bandwidth-bound streams whose few accumulators must stay in registers: no private (scratch) segment, no VGPR spill, no LDS (one wave
per block: nothing crosses a wave), and few enough registers for eight waves per SIMD."""
from test_code_object import _kernel_metadata


def test_prune_kernels_keep_their_state_in_registers(tmp_path):
    kernels = _kernel_metadata(tmp_path)
    pr = {n: m for n, m in kernels.items() if "vbs_prune_" in n}
    assert len(pr) == 2, sorted(pr)
    assert sum("vbs_prune_block_ssq_kernel" in n for n in pr) == 1 and sum("vbs_prune_mask_kernel" in n for n in pr) == 1
    for name, m in pr.items():
        assert m["private_segment_fixed_size"] == 0, (name, m)
        assert m["vgpr_spill_count"] == 0, (name, m)
        assert m["group_segment_fixed_size"] == 0, (name, m)
        assert m["vgpr_count"] <= 64, (name, m)                           # 512 / 64: eight waves per SIMD
        # (the step tests count the kernels of the steps, of set_values and of the products by these patterns)
        assert not any(p in name for p in ("vbs_adam_", "vbs_sgd_", "vbs_update_", "stream_kernel", "direct_kernel", "sddmm", "gradctl")), name
