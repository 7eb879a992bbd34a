"""The compiled gfx950 code object of the packed fp32 kernel (k_f32_packed.hip), checked without a GPU: like the direct kernel it keeps
its whole pipeline in registers (tests/test_code_object.py says why that is pinned), it asks for exactly the LDS of its `__shared__` array,
and it fits two workgroups per CU."""
import re

from tests.test_code_object import _disassemble, _kernel_metadata


def test_packed_kernel_keeps_its_state_in_registers(tmp_path):
    kernels = _kernel_metadata(tmp_path)
    pk = {n: m for n, m in kernels.items() if "vbs_spmm_f32_packed_kernel" in n}
    assert len(pk) == 4, sorted(pk)                                       # <CSTAGE, TAIL>
    plain = {n: m for n, m in pk.items() if "packed_kernelILb0E" in n}    # without the C ring: TAIL = true / false
    assert len(plain) == 2, sorted(pk)
    stage = 4 * 2 * 32 * 36 * 4                                           # 4 waves x 2 stages x 32 columns x (32 + 4) floats
    for name, m in pk.items():
        assert m["private_segment_fixed_size"] == 0, (name, m)            # no scratch
        assert m["vgpr_spill_count"] == 0, (name, m)
        assert m["vgpr_count"] <= 256, (name, m)                          # two 256-thread workgroups per CU
        want = stage if name in plain else stage + 4 * 32 * 65 * 4        # (+ the C ring: 4 waves x 32 columns x 65 floats)
        assert m["group_segment_fixed_size"] == want, (name, m, want)
        assert 2 * m["group_segment_fixed_size"] <= 160 * 1024, (name, m)


def test_packed_kernel_step_keeps_its_prefetch(tmp_path):
    """no scratch instruction; four wide LDS writes per group of a step instead of sixteen narrow ones; the step's waits leave a step's
    loads in flight (9 per step: 4 of B, 4 of A, 1 table) and a full wait appears only in the epilogue's C += path, never in a step of the loop"""
    ks = _disassemble(tmp_path)
    txts = [t for n, t in ks.items() if "vbs_spmm_f32_packed_kernelILb0E" in n]
    assert len(txts) == 2
    for txt in txts:
        ins = [l.split("//")[0].strip() for l in txt.splitlines() if l.startswith(("\t", " "))]
        ins = [i for i in ins if i]
        assert not any(i.startswith("scratch_") for i in ins)
        steps = sum(i.startswith("v_mfma") for i in ins) / 16
        assert 7 <= steps <= 12, steps
        assert not any(i.startswith("ds_write_b32") for i in ins)
        assert sum(i.startswith(("ds_write2_b64", "ds_write_b64")) for i in ins) <= 8 * (steps + 1)
        # a full wait belongs to the C += path of an epilogue: its 16 loads of C and no MFMA stand between it and the step's last MFMA.  The only others
        # are the countdown of the range's LAST step (nothing is requested behind it: vmcnt(2), (1), (0)), which the layout puts behind the loop's four bodies
        stray = []
        for k, i in enumerate(ins):
            if not re.match(r"s_waitcnt vmcnt\(0\)", i):
                continue
            back = ins[max(0, k - 40):k]
            last_mfma = max([j for j, b in enumerate(back) if b.startswith("v_mfma")], default=-1)
            if sum(bool(re.match(r"buffer_load_dword\s", b)) for b in back[last_mfma + 1:]) != 16:
                stray.append(sum(b.startswith("v_mfma") for b in ins[:k]))
        assert len(stray) <= 3 and all(n >= 4 * 16 for n in stray), stray      # (behind the 64 MFMAs of the loop's four step bodies)
        waits = [int(m.group(1)) for i in ins for m in [re.match(r"s_waitcnt vmcnt\((\d+)\)", i)] if m]
        assert sum(w >= 9 for w in waits) >= 4 * steps, (waits, steps)
