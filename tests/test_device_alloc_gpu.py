"""Who owns the device memory of a handle (sparta_amd/csrc/vbs_device.hpp: DevBuf, DevScratch, DevEvent), read through the two process-wide counters of
sparta_debug_device_allocs: every allocation a handle makes -- at creation, lazily at the first call of an entry, as scratch -- comes back when it is
destroyed; a second call of every entry allocates nothing; and the sizes a handle reports (info()["a_bytes"], a8_info()["image_bytes"]) are the ones the
library reported before its arrays had owners.

The handles: the four small training geometries of tests/_lifecycle.py (f16 w96, bf16 w128, f16 pair tiles, fp32 w13z), made updatable and transposable,
and the smallest matrices of tests/test_colres_gpu.py and tests/test_union_gpu.py through sparta_vbs_create_from_csr (the resident-column image, the sparse
rows, the column-compacted tiles).  Together they reach every group of device arrays a handle can hold."""
import ctypes as C

import numpy as np
import pytest

import sparta_amd as sa
from sparta_amd._lib import lib

import _lifecycle as L
from test_union_host import clustered, true_grouping

pytestmark = pytest.mark.gpu
f32 = np.float32
HANDLES = ["w96", "w128", "pairs_even", "w13z", "csr_colres", "csr_union"]
K = 8
# info()["a_bytes"] after creation, after the drive, and a8_info()["image_bytes"] after the drive, as the commit before the owning types printed them for the
# same handles and the same calls (profiles/device_alloc/README.md)
BEFORE = {"w96": (3162112, 3162112, 1581056), "w128": (2738176, 2738176, 1369088), "pairs_even": (294912, 294912, 147456), "w13z": (2048480, 2048480, 0),
          "csr_colres": (5120, 5120, 0), "csr_union": (543752, 543752, 0)}


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch


def allocs():
    n, b = C.c_int64(-1), C.c_int64(-1)
    assert lib.sparta_debug_device_allocs(C.byref(n), C.byref(b)) == 0
    return n.value, b.value


def open_handle(name, monkeypatch=None):
    """(handle, values or None): values = the mab array of a handle made from VBS arrays"""
    if name == "csr_colres":                                     # test_colres_gpu.py, SHAPES: the smallest
        from test_colres_gpu import _matrix, _handle
        return _handle(_matrix(63, 5, 0.6, 0, 68, 2))[0], None
    if name == "csr_union":                                      # test_union_gpu.py: the smallest clusters, at block width 1
        if monkeypatch is not None:                              # (a matrix this small would otherwise stay on one kind of launch)
            monkeypatch.setenv("SPARTA_SPARSE_MIN_STEPS", "0")
            monkeypatch.setenv("SPARTA_LAUNCH_NNZ", "0")
        m, order = clustered(40, 5, 5000, 100, 3, seed=16, integer=True)
        return sa.DeviceVBS.from_csr(m, true_grouping(order, 5), 1, device=0), None
    dtype = L.GEOS[name][0]
    v = L.geometry(name)
    W = np.random.default_rng(len(name)).uniform(-1, 1, int(v.nztot)).astype(f32)
    fresh = sa.VBR.from_arrays(v.rows, v.cols, v.block_col_size, v.row_part, v.nzcount, v.jab, W)
    return fresh.to_device(0, dtype=dtype, updatable=True, transposable=True), W


def drive(torch, h, W):
    """one call of every entry that builds something lazily or grows scratch, for what the handle is; leaves the switches as it found them.  Returns the
    PreparedB it made (the caller closes it)."""
    tdt = {sa.F32: torch.float32, sa.F16: torch.float16, sa.BF16: torch.bfloat16}[h.dtype]
    rows, cols = h.rows, h.cols
    rng = np.random.default_rng(rows + cols)
    h.set_class_timing(True)
    # products: host pointers; device pointers with n_cols % 128 != 0 (the column tail of a 16-bit handle); a prepared B; a gathered B where the shape has one
    n = 130
    Bh = rng.uniform(-1, 1, cols * n).astype(f32)
    Ch = np.zeros(rows * n, f32)
    h.spmm_host(Bh, K, Ch, accumulate=False)
    Bd = torch.from_numpy(Bh).cuda().to(tdt)
    Cd = torch.zeros(rows * n, dtype=torch.float32, device="cuda")
    h.spmm(Bd, Cd, n, timed=True)
    Bp = h.prepare_b(Bd, n)
    h.spmm_prepared(Bp, Cd)
    w = h.info()["block_col_size"]
    if cols % 2 == 0 and (cols // 2) % w == 0:
        h.spmm_gathered(Bd, cols // 2, Cd, n)                    # (any bytes will do for the slabs: nothing is compared)
    if W is not None:
        nb = h.n_blocks
        X = rng.uniform(-1, 1, rows * K).astype(f32)
        Y = rng.uniform(-1, 1, cols * K).astype(f32)
        G = np.zeros(W.size, f32)
        h.sddmm_host(X, Y, K, G, accumulate=False)
        Ct = np.zeros(cols * K, f32)
        h.spmm_t_host(X, K, Ct, accumulate=False)
        h.set_values_host(W)
        Wd = torch.from_numpy(W).cuda()
        h.block_ssq(Wd)
        keep = torch.ones(nb, dtype=torch.uint8, device="cuda")
        keep[::3] = 0
        h.set_live_blocks(keep)
        h.set_live_steps(True)
        h.set_live_forward(True)
        h.spmm(Bd, Cd, n)
        Xd, Yd = torch.from_numpy(X).cuda().to(tdt), torch.from_numpy(Y).cuda().to(tdt)
        h.sddmm_block_ssq(Xd, Yd, K)
        h.set_live_forward(False)
        if h.a8_info()["capable"]:
            h.set_forward_a8(True, values=Wd)
            h.set_a8_live(True)
            h.spmm(Bd, Cd, n)
            h.set_forward_a8(False)
        D = torch.empty_like(Wd)
        h.move_blocks(h, np.arange(nb, dtype=np.int32), (Wd, D))
        h.set_live_steps(False)
        h.set_live_blocks(None)
    torch.cuda.synchronize()
    return Bp


def figures(torch, name, monkeypatch=None):
    """what BEFORE holds for the handle: (a_bytes after creation, a_bytes after the drive, the fp8 image's bytes after the drive)"""
    h, W = open_handle(name, monkeypatch)
    try:
        created = h.info()["a_bytes"]
        drive(torch, h, W).close()
        return created, h.info()["a_bytes"], h.a8_info()["image_bytes"]
    finally:
        h.close()


@pytest.mark.parametrize("name", HANDLES)
def test_what_a_handle_allocates_comes_back(name, monkeypatch):
    torch = _torch()
    before = allocs()
    h, W = open_handle(name, monkeypatch)
    Bp = None
    try:
        created = allocs()
        assert created[0] > before[0] and created[1] > before[1], (before, created)
        Bp = drive(torch, h, W)
        driven = allocs()
        print("device allocations of %s: %s after creation, %s after every entry" % (name, created, driven))
        assert driven[0] > created[0] and driven[1] > created[1], (created, driven)
    finally:
        if Bp is not None:
            Bp.close()
        h.close()
    assert allocs() == before, "the handle or its prepared B kept device memory"


@pytest.mark.parametrize("name", HANDLES)
def test_steady_state_allocates_nothing(name, monkeypatch):
    torch = _torch()
    h, W = open_handle(name, monkeypatch)
    try:
        drive(torch, h, W).close()
        warm = allocs()
        drive(torch, h, W).close()
        assert allocs() == warm, "a second call of an entry allocated or freed device memory"
    finally:
        h.close()


@pytest.mark.parametrize("name", HANDLES)
def test_reported_bytes_are_those_before_the_owning_types(name, monkeypatch):
    torch = _torch()
    assert figures(torch, name, monkeypatch) == BEFORE[name]
