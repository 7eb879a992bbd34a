"""The compiled gfx950 code objects of k_dense.hip (sparta_dense_block_ssq / sparta_vbs_gather_dense / sparta_vbs_scatter_dense), checked without a GPU:
metadata fields only.  Bandwidth-bound copies and one reduction whose staged vectors and accumulators must stay in registers: no private (scratch)
segment, no VGPR spill, and exactly the LDS the source declares -- the transposing (row-major) kernels hold one 64 x 32 tile of words with a row stride of
33 per wave, four waves per workgroup; every other kernel none.  The names match none of the patterns other tests count kernels by."""
from test_code_object import _kernel_metadata
from test_repattern_code_object import FOREIGN

TILE_BYTES = 4 * 64 * 33 * 4          # kPruneWaves x kDnRows x kDnStride words


def test_the_dense_kernels_keep_their_state_in_registers(tmp_path):
    kernels = _kernel_metadata(tmp_path)
    dn = {n: m for n, m in kernels.items() if "vbs_dense_" in n}
    # element type x {gather, scatter} x {row-major, column-major}; the fill per element size; the score per element type and layout
    for stem, count in (("vbs_dense_gather_rm_kernel", 3), ("vbs_dense_gather_cm_kernel", 3), ("vbs_dense_scatter_rm_kernel", 3), ("vbs_dense_scatter_cm_kernel", 3),
                        ("vbs_dense_fill_kernel", 2), ("vbs_dense_ssq_kernel", 6)):
        assert sum(stem in n for n in dn) == count, (stem, sorted(dn))
    assert len(dn) == 20, sorted(dn)
    for name, m in dn.items():
        assert m["private_segment_fixed_size"] == 0, (name, m)
        assert m["vgpr_spill_count"] == 0, (name, m)
        assert m["group_segment_fixed_size"] == (TILE_BYTES if "_rm_kernel" in name else 0), (name, m)
        assert m["vgpr_count"] <= 128, (name, m)                          # at least four waves per SIMD
        assert not any(p in name for p in FOREIGN), name
        assert not any(p in name for p in ("vbs_repat_", "vbs_sddmm_")), name
