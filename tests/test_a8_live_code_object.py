"""The compiled gfx950 code objects of the fp8 image with a live-block set, checked without a GPU (metadata only): every kernel of the combined form
(vbs_fwdq8lv_h16_kernel, k_h16_a8_live.hip) is held to its plain sibling (vbs_spmm_h16_direct_kernel with the same template arguments) -- the documented set
of instantiations, which is the set of the a8 form, no scratch, no spill, the same LDS, a waves-per-SIMD class no lower -- and the scale-placement kernel
(vbs_q8lv_scales_kernel) is one instantiation that uses registers only."""
from test_code_object import _kernel_metadata
from test_live_forward_code_object import _args, _waves_per_simd

Q8LV, PLAIN, SCALES = "vbs_fwdq8lv_h16_kernel", "vbs_spmm_h16_direct_kernel", "vbs_q8lv_scales_kernel"


def test_a8_live_kernels_match_their_plain_siblings(tmp_path):
    kernels = _kernel_metadata(tmp_path)
    mine = {_args(n, Q8LV): (n, m) for n, m in kernels.items() if Q8LV in n}
    plain = {_args(n, PLAIN): (n, m) for n, m in kernels.items() if PLAIN in n}
    want = set()                                                                       # <KP, MI2, BF16, GATHERED, CSTAGE, DEEP, TAIL, WC, SLAB>
    for bf16 in "01":
        for tail in "01":
            for kp in ("32", "64"):
                for cstage in "01":
                    want.add((kp, "0", bf16, "0", cstage, "0", tail, "32", "0"))       # one tile, 32-column waves, with and without the C ring
                want.add((kp, "1", bf16, "0", "0", "0", tail, "32", "0"))              # pair / 64-row tiles
            want.add(("32", "0", bf16, "0", "0", "0", tail, "64", "0"))                # 64-column waves (two sub-workers per workgroup)
    assert len(want) == 28
    assert len([n for n in kernels if Q8LV in n]) == 28
    assert set(mine) == want, sorted(set(mine) ^ want)                                 # (no 256-column slab, no four-accumulator form: DESIGN.md 3.18)
    for args, (name, m) in sorted(mine.items()):
        assert args in plain, ("no plain sibling", name)
        pn, pm = plain[args]
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m.get("sgpr_spill_count", 0) == 0, (name, m)
        assert m["group_segment_fixed_size"] == pm["group_segment_fixed_size"], (name, m, pm)
        assert m["vgpr_count"] <= 256, (name, m)
        assert _waves_per_simd(m["vgpr_count"]) >= _waves_per_simd(pm["vgpr_count"]), (name, m["vgpr_count"], pn, pm["vgpr_count"])


def test_scale_placement_kernel_uses_registers_only(tmp_path):
    kernels = _kernel_metadata(tmp_path)
    sk = {n: m for n, m in kernels.items() if SCALES in n}
    assert len(sk) == 1, sorted(sk)
    for name, m in sk.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m.get("sgpr_spill_count", 0) == 0, (name, m)
        assert m["group_segment_fixed_size"] == 0, (name, m)
        assert m["vgpr_count"] <= 128, (name, m)
    # the names stay clear of what the other code-object tests count
    for n in kernels:
        if Q8LV in n or SCALES in n:
            assert not any(s in n for s in ("stream_kernel", "direct_kernel", "vbs_live_", "vbs_update_", "vbs_sgd_", "vbs_adam_", "vbs_fwdlive_", "live_blocks_kernel",
                                            "vbs_fwda8_h16_kernel", "vbs_a8quant_kernel", "vbs_lvstep_words_kernel")), n
