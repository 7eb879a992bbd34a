"""The compiled gfx950 code objects of the live forward product, checked without a GPU: every live kernel (vbs_fwdlive_h16_kernel, k_h16_live.hip) is held
to its plain sibling (vbs_spmm_h16_direct_kernel with the same template arguments) -- no scratch, no spill, the same LDS, a register count in the
waves-per-SIMD class of the sibling, at most 512 registers for the four-accumulator form and 256 otherwise -- and the compaction kernel (k_live.hip) uses
registers only.  "In the class of the sibling" is checked as "no lower": the one-tile KP = 64 TAIL instantiations take 128 registers where the plain ones
take 143 (four waves per SIMD instead of three), which is no loss; every other instantiation lands in the very class of its sibling."""
import re

from test_code_object import _kernel_metadata

LIVE, PLAIN, COMPACT = "vbs_fwdlive_h16_kernel", "vbs_spmm_h16_direct_kernel", "vbs_fwdlive_compact_kernel"


def _waves_per_simd(vgprs):
    """512 registers per lane and SIMD, allocated in blocks of 8; at most 8 waves"""
    return min(8, 512 // max(8, (vgprs + 7) // 8 * 8))


def _args(name, kernel):
    """the mangled template arguments of an instantiation: <KP, MI2, BF16, GATHERED, CSTAGE, DEEP, TAIL, WC, SLAB>"""
    tail = name.split(kernel, 1)[1]
    return tuple(re.findall(r"L[ib](\d+)E", tail.split("EEvN10sparta_dev")[0]))


def test_live_kernels_match_their_plain_siblings(tmp_path):
    kernels = _kernel_metadata(tmp_path)
    live = {_args(n, LIVE): (n, m) for n, m in kernels.items() if LIVE in n}
    plain = {_args(n, PLAIN): (n, m) for n, m in kernels.items() if PLAIN in n}
    want = set()
    for bf16 in "01":
        for tail in "01":
            for kp in ("32", "64"):
                for cstage in "01":
                    want.add((kp, "0", bf16, "0", cstage, "0", tail, "32", "0"))       # one tile, 32-column waves, with and without the C ring
                want.add((kp, "1", bf16, "0", "0", "0", tail, "32", "0"))              # pair / 64-row tiles
                want.add((kp, "1", bf16, "0", "0", "0", tail, "64", "1"))              # four accumulators per wave over 256-column slabs
            want.add(("32", "0", bf16, "0", "0", "0", tail, "64", "0"))                # 64-column waves (two sub-workers per workgroup)
            want.add(("32", "0", bf16, "0", "0", "0", tail, "64", "1"))                # the 256-column slab form
    assert set(live) == want, sorted(set(live) ^ want)
    for args, (name, m) in sorted(live.items()):
        assert args in plain, ("no plain sibling", name)
        pn, pm = plain[args]
        assert len(args) == 9, name
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (name, m)
        assert m["group_segment_fixed_size"] == pm["group_segment_fixed_size"], (name, m, pm)
        quad = args[1] == "1" and args[7] == "64"
        assert m["vgpr_count"] <= (512 if quad else 256), (name, m)
        assert _waves_per_simd(m["vgpr_count"]) >= _waves_per_simd(pm["vgpr_count"]), (name, m["vgpr_count"], pn, pm["vgpr_count"])


def test_compaction_kernel_uses_registers_only(tmp_path):
    kernels = _kernel_metadata(tmp_path)
    ck = {n: m for n, m in kernels.items() if COMPACT in n}
    assert len(ck) == 1, sorted(ck)
    for name, m in ck.items():
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["group_segment_fixed_size"] == 0, (name, m)
        assert m["vgpr_count"] <= 128, (name, m)
    # the names stay clear of what the other code-object tests count
    for n in kernels:
        if LIVE in n or COMPACT in n:
            assert not any(s in n for s in ("stream_kernel", "direct_kernel", "vbs_live_", "vbs_lvstep_words_kernel", "live_blocks_kernel")), n
