"""sparta_vbs_sddmm (SDDMM on the stored blocks of a handle, k_sddmm.hip) without a GPU: the entry is exported, refuses NULL arguments with a
message, and its kernels keep their state in registers (no scratch, no VGPR spills)."""
import ctypes as C

import sparta_amd  # noqa: F401  (loads the library)
from sparta_amd import _lib
from sparta_amd._lib import lib

from test_code_object import _kernel_metadata


def test_sddmm_symbol_exported():
    assert "sparta_vbs_sddmm" in _lib.SYMBOLS
    assert hasattr(lib, "sparta_vbs_sddmm")


def test_sddmm_null_handle_is_invalid():
    G = (C.c_float * 4)()
    rc = lib.sparta_vbs_sddmm(None, None, 1, None, 1, 1, G, 0, _lib.PTR_DEVICE, None, None)
    assert rc == _lib.ERR_INVALID
    msg = lib.sparta_last_error().decode()
    assert "sparta_vbs_sddmm" in msg and "NULL" in msg, msg


def test_sddmm_kernels_have_no_scratch_and_no_spills(tmp_path):
    kernels = _kernel_metadata(tmp_path)
    sd = {n: m for n, m in kernels.items() if "sddmm" in n}
    assert len(sd) == 5, sorted(sd)                     # fp32; fp16 and bf16, each with and without the 16-byte loads of Y
    for name, m in sd.items():
        assert m["private_segment_fixed_size"] == 0, (name, m)
        assert m["vgpr_spill_count"] == 0, (name, m)
        assert m["group_segment_fixed_size"] % 16 == 0, (name, m)     # (the 16-bit kernels' transposed reads need a 16-byte aligned image)
