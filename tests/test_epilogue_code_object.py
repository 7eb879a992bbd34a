"""The compiled gfx950 code object of the kernels of k_epilogue.hip (sparta_epilogue_fwd / sparta_epilogue_bwd), checked without a GPU: metadata fields only.
Both element kernels are bandwidth-bound streams: the loads of four columns in flight, the bias and (backward) nothing else must stay in registers -- no
private (scratch) segment, no VGPR spill, at most 128 registers (four waves per SIMD) -- and the only LDS is the 32 x 256 floats the backward kernel parks
its fp32 dz in for the bias gradient."""
from test_code_object import _kernel_metadata

OTHERS = ("vbs_adam_", "vbs_sgd_", "vbs_update_", "vbs_prune_", "stream_kernel", "direct_kernel", "sddmm", "gradctl", "live")   # other tests count kernels by these


def test_epilogue_kernels_keep_their_state_in_registers(tmp_path):
    kernels = _kernel_metadata(tmp_path)
    ep = {n: m for n, m in kernels.items() if "vbs_epilogue_" in n}
    # forward: one per output type; backward: one per (dY type, dZ type); the fold of the run sums
    assert sum("vbs_epilogue_fwd_kernel" in n for n in ep) == 3, sorted(ep)
    assert sum("vbs_epilogue_bwd_kernel" in n for n in ep) == 9, sorted(ep)
    assert sum("vbs_epilogue_fold_kernel" in n for n in ep) == 1, sorted(ep)
    assert len(ep) == 13, sorted(ep)
    for name, m in ep.items():
        assert m["private_segment_fixed_size"] == 0, (name, m)
        assert m["vgpr_spill_count"] == 0, (name, m)
        assert m["vgpr_count"] <= 128, (name, m)
        assert m["group_segment_fixed_size"] == (32 * 256 * 4 if "bwd_kernel" in name else 0), (name, m)
        assert not any(p in name for p in OTHERS), name
