"""sparta_vbs_set_values (new values for an updatable handle, k_update.hip) without a GPU: the entries are exported, a NULL handle is refused with a
message, the update kernels keep their state in registers, and the k-compaction rule the host packer and the update kernel share
(frag_position / frag_pairs behind sparta_frag_positions) does what DESIGN.md section 3.5 says."""
import ctypes as C

import numpy as np

import sparta_amd  # noqa: F401  (loads the library)
from sparta_amd import _lib
from sparta_amd._lib import lib

from test_code_object import _kernel_metadata

NEW = ["sparta_vbs_create_range_ex", "sparta_vbs_set_values", "sparta_vbs_flags", "sparta_frag_positions"]


def test_set_values_symbols_exported():
    for s in NEW:
        assert s in _lib.SYMBOLS, s
        assert hasattr(lib, s), s


def test_set_values_null_handle_is_invalid():
    mab = (C.c_float * 4)()
    rc = lib.sparta_vbs_set_values(None, mab, _lib.PTR_DEVICE, None, None)
    assert rc == _lib.ERR_INVALID
    msg = lib.sparta_last_error().decode()
    assert "sparta_vbs_set_values" in msg and "NULL" in msg, msg
    f = C.c_int32(7)
    assert lib.sparta_vbs_flags(None, C.byref(f)) == _lib.ERR_INVALID
    assert "sparta_vbs_flags" in lib.sparta_last_error().decode()


def test_update_kernels_have_no_scratch_and_no_spills(tmp_path):
    kernels = _kernel_metadata(tmp_path)
    up = {n: m for n, m in kernels.items() if "vbs_update_" in n}
    # the copy, the fp32 fragment kernel, and the 16-bit slice kernel for {f16, bf16} x {32x32, 64x32, 32x64, 64x64 slices, hub slices}
    assert len(up) == 12, sorted(up)
    assert sum("vbs_update_f32_frag_kernel" in n for n in up) == 1 and sum("vbs_update_h16_kernel" in n for n in up) == 10
    for name, m in up.items():
        assert m["private_segment_fixed_size"] == 0, (name, m)
        assert m["vgpr_spill_count"] == 0, (name, m)
        assert not any(p in name for p in ("stream_kernel", "direct_kernel", "sddmm")), name     # (test_code_object.py counts kernels by these patterns)


def _positions(mask):
    ne = (C.c_uint8 * 32)(*[int(b) for b in mask])
    pos = (C.c_uint8 * 32)()
    pairs = C.c_int32(-1)
    assert lib.sparta_frag_positions(ne, pos, C.byref(pairs)) == _lib.OK
    return np.array(pos[:], np.int64), int(pairs.value)


def _reference_positions(mask):
    """the rule as vbs_plan.cpp stated it before it was shared: class by class (k = 4 m + ((e + m) & 3)), non-empty columns first"""
    order = []
    for want in (True, False):
        for m in range(8):
            for e in range(4):
                k = 4 * m + ((e + m) & 3)
                if bool(mask[k]) == want:
                    order.append(k)
    pos = np.zeros(32, np.int64)
    for c, k in enumerate(order):
        pos[k] = (c >> 1) + 16 * (c & 1)
    return pos


def test_frag_positions_rule():
    rng = np.random.default_rng(20261016)
    masks = [np.zeros(32, bool), np.ones(32, bool)]
    masks += [rng.random(32) < p for p in rng.uniform(0.02, 0.98, 1000)]
    masks += [np.arange(32) == k for k in range(32)]
    for mask in masks:
        pos, pairs = _positions(mask)
        nk = int(mask.sum())
        assert sorted(pos.tolist()) == list(range(32)), (mask, pos)
        compact = 2 * (pos % 16) + pos // 16                       # c sits at pos = (c >> 1) + 16 (c & 1)
        assert np.all(compact[mask] < nk) and np.all(compact[~mask] >= nk), (mask, pos)
        assert pairs == (max(1, (nk + 1) // 2) + 1) // 2, (mask, pairs)
        assert np.array_equal(pos, _reference_positions(mask)), (mask, pos)
    assert lib.sparta_frag_positions(None, None, None) == _lib.ERR_INVALID
