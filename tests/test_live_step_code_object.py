"""The gfx950 code objects of the live steps, checked without a GPU (metadata through _kernel_metadata of tests/test_code_object.py, instructions through
its _disassemble).

The live image kernels (vbs_sgdlive_* / vbs_adamlive_*, k_update_image.inc compiled once more per stepping source) must stay in the occupancy class of
their plain siblings: no scratch, no spill, the same LDS, and a register count that allows the same number of waves per SIMD (512 registers per lane and
SIMD, allocated in units of 8, at most 8 waves).  The kernels of the two-pass form and the kernel that writes the live words are register-only.  The plain
kernels keep their names and counts: the names of the live ones avoid "vbs_sgd_", "vbs_adam_", "vbs_update_" and "vbs_live_", by which other tests count."""
from test_code_object import _disassemble, _kernel_metadata


def _waves(vgprs):
    return min(8, 512 // (max((vgprs + 7) // 8, 1) * 8))


def _siblings(kernels, live_tag, plain_tag):
    live = {n: m for n, m in kernels.items() if live_tag in n and "blocks_kernel" not in n}       # (the two-pass kernels have no sibling of their shape)
    plain = {n: m for n, m in kernels.items() if plain_tag in n}
    pairs = []
    for name, m in live.items():
        # "f32_frag_kernelE" or "h16_kernelILb.ELi..ELi..EEEv": the kernel and its template arguments, up to the first argument type
        form = name.split(live_tag)[1].split("PNS_")[0].split("PKNS_")[0]
        cands = [n for n in plain if (plain_tag + form) in n]
        assert len(cands) == 1, (name, form, sorted(plain))
        pairs.append((name, m, cands[0], plain[cands[0]]))
    return pairs


def test_live_image_kernels_match_their_siblings(tmp_path):
    kernels = _kernel_metadata(tmp_path)
    for live_tag, plain_tag in (("vbs_sgdlive_", "vbs_sgd_"), ("vbs_adamlive_", "vbs_adam_")):
        pairs = _siblings(kernels, live_tag, plain_tag)
        assert len(pairs) == 9, [p[0] for p in pairs]                   # the fp32 fragment kernel + h16<BF16, TMS, KP> x 8
        assert sum("f32_frag_kernel" in p[0] for p in pairs) == 1 and sum("h16_kernelILb" in p[0] for p in pairs) == 8
        for name, m, sib, s in pairs:
            assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (name, m)
            assert s["private_segment_fixed_size"] == 0 and s["vgpr_spill_count"] == 0, (sib, s)
            assert m["group_segment_fixed_size"] == s["group_segment_fixed_size"], (name, m, s)
            assert _waves(m["vgpr_count"]) == _waves(s["vgpr_count"]), (name, m["vgpr_count"], s["vgpr_count"])


def test_blocks_kernels_and_word_kernel_use_registers_only(tmp_path):
    kernels = _kernel_metadata(tmp_path)
    ks = {n: m for n, m in kernels.items() if "live_blocks_kernel" in n or "vbs_lvstep_words_kernel" in n}
    assert len(ks) == 3 and sum("vbs_sgdlive_blocks_kernel" in n for n in ks) == 1 and sum("vbs_adamlive_blocks_kernel" in n for n in ks) == 1, sorted(ks)
    for name, m in ks.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["group_segment_fixed_size"] == 0, (name, m)


def test_plain_kernels_keep_their_names_and_counts(tmp_path):
    kernels = _kernel_metadata(tmp_path)
    assert sum("vbs_sgd_" in n for n in kernels) == 10 and sum("vbs_adam_" in n for n in kernels) == 11
    assert sum("vbs_update_" in n for n in kernels) == 12 and sum("vbs_live_" in n for n in kernels) == 2
    for part, count in (("vbs_sgd_step_kernel", 1), ("vbs_sgd_f32_frag_kernel", 1), ("vbs_sgd_h16_kernelILb", 8), ("vbs_adam_tick_kernel", 1),
                        ("vbs_adam_step_kernel", 1), ("vbs_adam_f32_frag_kernel", 1), ("vbs_adam_h16_kernelILb", 8)):
        assert sum(part in n for n in kernels) == count, part
    assert sum("vbs_sgdlive_" in n for n in kernels) == 10 and sum("vbs_adamlive_" in n for n in kernels) == 10


def test_live_kernels_round_once_per_operation(tmp_path):
    """the arithmetic of the live forms is the pinned one: multiplies and adds, no fused multiply-add (as tests/test_sgd_step_host.py holds the plain ones)"""
    txt = {n: t for n, t in _disassemble(tmp_path).items() if "vbs_sgdlive_" in n or "vbs_adamlive_" in n}
    assert len(txt) == 20, sorted(txt)
    fused = ("v_fma_f32", "v_fmac_f32", "v_mac_f32", "v_mad_f32", "v_pk_fma_f32", "v_fma_mix", "v_mad_legacy_f32", "v_fma_legacy_f32")
    for name, t in txt.items():
        ins = [ln.split()[0] for ln in t.splitlines() if ln.strip()]
        assert any(i.startswith("v_mul_f32") or i.startswith("v_pk_mul_f32") for i in ins), name
        if "vbs_sgdlive_" in name:                                     # (the Adam kernels' division and square root expand to sequences with FMAs: not pinned here either)
            assert not [i for i in ins if i.startswith(fused)], name
