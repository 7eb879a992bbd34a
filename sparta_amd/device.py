"""Device side: VBS image on one MI355X and the fused SpMM (sparta_vbs_create / sparta_vbs_spmm)."""
import ctypes as C
import numpy as np

from . import _lib
from ._lib import lib, check

_i64p = C.POINTER(C.c_int64)
_f32p = C.POINTER(C.c_float)


def _ctl_ptr(ctl, device):
    """the device address of a control record: a sparta_amd.GradCtl, its tensor (GRAD_CTL_BYTES on this device), or None"""
    if ctl is None:
        return None
    R = getattr(ctl, "R", ctl)
    if not (R.is_cuda and R.device.index == device and R.is_contiguous() and R.numel() * R.element_size() >= _lib.GRAD_CTL_BYTES):
        raise ValueError("ctl must be a GradCtl, or a contiguous tensor of GRAD_CTL_BYTES = %d bytes, on device %d" % (_lib.GRAD_CTL_BYTES, device))
    return C.c_void_p(R.data_ptr())


def device_count():
    return int(lib.sparta_device_count())


class _Info(dict):
    """An info dict that grew: the words an entry point reported from the start are its items -- equality, iteration and len() see those alone, as code that
    compares whole dicts expects -- and the words added later answer to subscript and get()."""

    def __init__(self, items, later):
        super().__init__(items)
        self.later = dict(later)

    def __missing__(self, key):
        return self.later[key]

    def get(self, key, default=None):
        return self[key] if key in self or key in self.later else default

    def __repr__(self):
        return "%s + %r" % (dict.__repr__(self), self.later)


class ValuesRecord:
    """vbs_linear's record, kept on a handle, of which tensor (at which version) the handle's values were last taken from (autograd.py).  Whatever
    gives the handle other values, or none, calls _values_replaced(); a handle class of its own that vbs_linear is to drive derives from this."""
    _autograd_values = None                    # (tensor, version) or None
    _autograd_captured = False                 # a forward was recorded into a graph: replays change the values unseen, so nothing is skipped any more

    def _values_replaced(self):
        self._autograd_values = None


class DeviceVBS(ValuesRecord):
    """Opaque device image of a VBS matrix + its tile plan (sparta_vbs_t)."""

    def __init__(self, vbmat, device=0, dtype=_lib.F32, block_row_range=None, updatable=False, transposable=False):
        """updatable=True (SPARTA_CREATE_UPDATABLE): the handle takes new values for the same block pattern through set_values; it keeps every
        block-row on the dense-block kernels (none moves to the sparse-row kernels).  transposable=True (SPARTA_CREATE_TRANSPOSE): the handle
        also takes spmm_t (Ct = A^T X on its own blocks); its forward product is that of a plain handle."""
        self.device = int(device)
        self.dtype = dtype
        self.h = C.c_void_p(None)
        if vbmat is None:                      # from_csr fills the handle
            return
        rp = np.ascontiguousarray(vbmat.row_part, np.int64)
        nz = np.ascontiguousarray(vbmat.nzcount, np.int64)
        jab = np.ascontiguousarray(vbmat.jab, np.int64)
        mab = np.ascontiguousarray(vbmat.mab, np.float32)
        b0, b1 = (0, vbmat.block_rows) if block_row_range is None else block_row_range
        check(lib.sparta_vbs_create_range_ex(C.byref(self.h), vbmat.rows, vbmat.cols, vbmat.block_rows, vbmat.block_col_size,
                                             rp.ctypes.data_as(_i64p), nz.ctypes.data_as(_i64p), jab.ctypes.data_as(_i64p),
                                             mab.ctypes.data_as(_f32p), int(b0), int(b1), int(dtype), self.device,
                                             (_lib.CREATE_UPDATABLE if updatable else 0) | (_lib.CREATE_TRANSPOSE if transposable else 0)))
        info = self.info()
        self.rows, self.cols = info["rows"], info["cols"]

    @classmethod
    def from_csr(cls, cmat, grouping, col_block_size, row_block_size=0, force_fixed_size=False, device=0, dtype=_lib.F32):
        """sparta_vbs_create_from_csr: build + upload in one step without expanding the nearly empty block-rows into dense blocks
        (what makes 10^8-nonzero power-law matrices fit); same product as VBR().fill_from_CSR_inplace(...).to_device()."""
        self = cls(None, device=device, dtype=dtype)
        g = np.ascontiguousarray(grouping, np.int64)
        if g.shape != (cmat.rows,):
            raise ValueError("grouping must have one entry per row")
        rp = np.ascontiguousarray(cmat.rowptr, np.int64)
        ci = np.ascontiguousarray(cmat.colidx, np.int32)
        vals = None if cmat.vals is None else np.ascontiguousarray(cmat.vals, np.float32)
        check(lib.sparta_vbs_create_from_csr(C.byref(self.h), cmat.rows, cmat.cols, rp.ctypes.data_as(_i64p), ci.ctypes.data_as(C.POINTER(C.c_int32)),
                                             None if vals is None else vals.ctypes.data_as(_f32p), g.ctypes.data_as(_i64p), int(col_block_size),
                                             int(row_block_size), int(bool(force_fixed_size)), int(dtype), self.device))
        info = self.info()
        self.rows, self.cols = info["rows"], info["cols"]
        return self

    @staticmethod
    def plan_stats(cmat, grouping, col_block_size, row_block_size=0, force_fixed_size=False, dtype=_lib.F32):
        """sparta_vbs_plan_stats: what from_csr WOULD build for this grouping (no GPU, nothing built): tiles, their area and MFMA
        steps, and what is left to the sparse-row kernels."""
        g = np.ascontiguousarray(grouping, np.int64)
        if g.shape != (cmat.rows,):
            raise ValueError("grouping must have one entry per row")
        rp = np.ascontiguousarray(cmat.rowptr, np.int64)
        ci = np.ascontiguousarray(cmat.colidx, np.int32)
        vals = None if cmat.vals is None else np.ascontiguousarray(cmat.vals, np.float32)
        st = np.zeros(8, np.int64)
        check(lib.sparta_vbs_plan_stats(cmat.rows, cmat.cols, rp.ctypes.data_as(_i64p), ci.ctypes.data_as(C.POINTER(C.c_int32)),
                                        None if vals is None else vals.ctypes.data_as(_f32p), g.ctypes.data_as(_i64p), int(col_block_size),
                                        int(row_block_size), int(bool(force_fixed_size)), int(dtype), st.ctypes.data_as(_i64p)))
        keys = ["tile_blocks", "tile_area", "mfma_steps", "sparse_nnz", "sparse_rows", "block_rows", "rows", "union_steps"]
        return {k: int(st[i]) for i, k in enumerate(keys)}

    @staticmethod
    def predict_cost(cmat, grouping, col_block_size, row_block_size=0, force_fixed_size=False, dtype=_lib.F32, n_cols=128):
        """Predicted time of one product of the handle from_csr would build (plan_stats x measured rates on one MI355X): the dense tiles at
        the executed rate of the stream kernels on power-law hubs (16-bit: 220 TFLOP/s = 13.6 ms for 5.8e9 stored elements x 256 columns;
        fp32: 100), the sparse rows at the gather rate (one n_cols-wide row of B per nonzero: 5.9 TB/s when every gather goes to HBM, 9.5 TB/s
        where the library takes the long rows column window by column window -- from 262144 columns and 4 M nonzeros, vbs_capi.cpp)
        + their rows of C.  Good to ~10 % on R-MAT parts (profiles/r3): enough to choose between two blockings of one matrix, which is all it is for."""
        st = DeviceVBS.plan_stats(cmat, grouping, col_block_size, row_block_size, force_fixed_size, dtype)
        esz = 4.0 if dtype == _lib.F32 else 2.0
        t_tiles = 2.0 * st["tile_area"] * n_cols / ((100e12 if dtype == _lib.F32 else 220e12))
        rate = 9.5e12 if (cmat.cols >= 4 * 65536 and st["sparse_nnz"] >= (4 << 20)) else 5.9e12
        t_sparse = st["sparse_nnz"] * (n_cols * esz + 8.0) / rate + st["sparse_rows"] * n_cols * 4.0 / 5.9e12
        st["ms_tiles"], st["ms_sparse"] = t_tiles * 1e3, t_sparse * 1e3
        st["ms"] = (t_tiles + t_sparse) * 1e3
        return st

    @classmethod
    def transposed_of(cls, vbmat, device=0, dtype=_lib.F32):
        """sparta_vbs_create_transposed: the handle of A^T, for the B * A product (spmm_BA)"""
        self = cls(None, device=device, dtype=dtype)
        rp = np.ascontiguousarray(vbmat.row_part, np.int64)
        nz = np.ascontiguousarray(vbmat.nzcount, np.int64)
        jab = np.ascontiguousarray(vbmat.jab, np.int64)
        mab = np.ascontiguousarray(vbmat.mab, np.float32)
        check(lib.sparta_vbs_create_transposed(C.byref(self.h), vbmat.rows, vbmat.cols, vbmat.block_rows, vbmat.block_col_size,
                                               rp.ctypes.data_as(_i64p), nz.ctypes.data_as(_i64p), jab.ctypes.data_as(_i64p),
                                               mab.ctypes.data_as(_f32p), int(dtype), self.device))
        info = self.info()
        self.rows, self.cols = info["rows"], info["cols"]          # rows = cols(A), cols = rows(A)
        return self

    def spmm_BA_host(self, B, M, C_out, accumulate=True):
        """C (+)= B * A on the handle of A^T, host buffers: B is M x rows(A), C is M x cols(A), both column-major (ld = M).  Returns kernel ms."""
        B = np.ascontiguousarray(B, np.float32).reshape(-1)
        if not (isinstance(C_out, np.ndarray) and C_out.dtype == np.float32 and C_out.flags.c_contiguous):
            raise ValueError("C must be a contiguous float32 numpy array (it is written in place)")
        if B.size < M * self.cols or C_out.size < M * self.rows:
            raise ValueError("B or C too small")
        dt = C.c_float(0)
        check(lib.sparta_vbs_spmm_ba(self.h, B.ctypes.data_as(C.c_void_p), int(M), int(M), C_out.ctypes.data_as(C.c_void_p), int(M),
                                     int(bool(accumulate)), _lib.PTR_HOST, None, C.byref(dt)))
        return dt.value

    def info(self):
        a = np.zeros(16, np.int64)
        check(lib.sparta_vbs_info(self.h, a.ctypes.data_as(_i64p)))
        keys = ["rows", "cols", "block_rows", "block_col_size", "nblocks", "nztot", "tiles16", "tiles32", "tiles64",
                "sparse_rows", "a_bytes", "exec_area", "stream_steps", "stream_workers", "split_tiles", "last_path"]
        return {k: int(a[i]) for i, k in enumerate(keys)}

    def packed_info(self):
        """the packed plan of an fp32 handle (k_f32_packed.hip): see sparta_vbs_packed_info"""
        a = np.zeros(4, np.int64)
        check(lib.sparta_vbs_packed_info(self.h, a.ctypes.data_as(_i64p)))
        return {"packed": int(a[0]), "steps": int(a[1]), "slots": int(a[2]), "block_steps": int(a[3])}

    def sparse_info(self):
        """the part of the matrix on the sparse-row path: rows, nonzeros, rows handled by one wave, hub rows"""
        a = np.zeros(4, np.int64)
        check(lib.sparta_vbs_sparse_info(self.h, a.ctypes.data_as(_i64p)))
        return {"rows": int(a[0]), "nnz": int(a[1]), "short_rows": int(a[2]), "hub_rows": int(a[3])}

    def colres_info(self):
        """the resident-column image of a small fp32 handle (k_colres.hip): see sparta_vbs_colres_info; "nc" = columns per workgroup of the last product on that path"""
        a = np.zeros(12, np.int64)
        check(lib.sparta_vbs_colres_info(self.h, a.ctypes.data_as(_i64p)))
        return {"slices": int(a[0]), "entries": int(a[1]), "long_rows": int(a[2]), "plane": int(a[3]), "lmax": int(a[4]), "nc": int(a[5]), "nnz": int(a[6]), "unit": int(a[7]),
                "parts": int(a[8]), "ranges": int(a[9]), "small_parts": int(a[10]), "used_small": int(a[11])}

    def union_info(self):
        """the column-compacted ("union-pattern") tiles of a handle made from a CSR (k_union.hip): see sparta_vbs_union_info"""
        a = np.zeros(12, np.int64)
        check(lib.sparta_vbs_union_info(self.h, a.ctypes.data_as(_i64p)))
        keys = ["tiles32", "tiles64", "steps32", "steps64", "area", "list_entries", "nnz", "workers", "rows", "tail_nnz", "exec_area", "row_tile"]
        return {k: int(a[i]) for i, k in enumerate(keys)}

    def hub_info(self):
        """the hub part of a 16-bit plan (group tiles of long 64-row tiles for the GEMM-shaped kernel): see sparta_vbs_hub_info"""
        a = np.zeros(10, np.int64)
        check(lib.sparta_vbs_hub_info(self.h, a.ctypes.data_as(_i64p)))
        keys = ["steps", "tiles", "groups", "tiles_per_group", "stored_area", "union_area", "workers", "chunks", "segments"]
        return {k: int(a[i]) for i, k in enumerate(keys)}

    def spmm_host(self, B, n_cols, C_out, accumulate=True, algo=_lib.SPMM_MFMA, b_layout=_lib.COL_MAJOR,
                  c_layout=_lib.COL_MAJOR):
        """Host buffers in, host buffers out (the reference back-ends' contract). Returns kernel ms."""
        B = np.ascontiguousarray(B, np.float32).reshape(-1)
        if not (isinstance(C_out, np.ndarray) and C_out.dtype == np.float32 and C_out.flags.c_contiguous):
            raise ValueError("C must be a contiguous float32 numpy array (it is written in place)")
        ldb = self.cols if b_layout == _lib.COL_MAJOR else n_cols
        ldc = self.rows if c_layout == _lib.COL_MAJOR else n_cols
        if B.size < self.cols * n_cols or C_out.size < self.rows * n_cols:
            raise ValueError("B or C too small")
        dt = C.c_float(0)
        check(lib.sparta_vbs_spmm(self.h, B.ctypes.data_as(C.c_void_p), ldb, b_layout, int(n_cols),
                                  C_out.ctypes.data_as(C.c_void_p), ldc, c_layout, int(bool(accumulate)), _lib.PTR_HOST, None,
                                  int(algo), C.byref(dt)))
        return dt.value

    def spmm(self, B, C_out, n_cols, accumulate=False, algo=_lib.SPMM_MFMA, b_layout=_lib.COL_MAJOR, c_layout=_lib.COL_MAJOR,
             ldb=None, ldc=None, timed=False, stream=None):
        """Device tensors (torch, on this device): stream-ordered on torch's current stream, no copies.
        B: cols x n_cols, C: rows x n_cols in the given layouts. Returns kernel ms if timed else None.
        Handles created with dtype F16 / BF16 take B in that type (column-major, even ldb); C is always float32."""
        import torch
        want_b = {_lib.F32: torch.float32, _lib.F16: torch.float16, _lib.BF16: torch.bfloat16}[self.dtype]
        if not (B.is_cuda and C_out.is_cuda and B.dtype == want_b and C_out.dtype == torch.float32):
            raise ValueError("B must be a %s tensor and C a float32 tensor, both on the GPU" % want_b)
        if B.device.index != self.device or C_out.device.index != self.device:
            raise ValueError("B and C must live on device %d" % self.device)
        ldb = (self.cols if b_layout == _lib.COL_MAJOR else n_cols) if ldb is None else ldb
        ldc = (self.rows if c_layout == _lib.COL_MAJOR else n_cols) if ldc is None else ldc
        need_b = ldb * (n_cols if b_layout == _lib.COL_MAJOR else self.cols)
        need_c = ldc * (n_cols if c_layout == _lib.COL_MAJOR else self.rows)
        if B.numel() < need_b or C_out.numel() < need_c or not B.is_contiguous() or not C_out.is_contiguous():
            raise ValueError("B or C too small / not contiguous for the stated leading dimensions")
        st = torch.cuda.current_stream(self.device).cuda_stream if stream is None else stream
        dt = C.c_float(0)
        check(lib.sparta_vbs_spmm(self.h, C.c_void_p(B.data_ptr()), int(ldb), b_layout, int(n_cols), C.c_void_p(C_out.data_ptr()),
                                  int(ldc), c_layout, int(bool(accumulate)), _lib.PTR_DEVICE, C.c_void_p(st), int(algo),
                                  C.byref(dt) if timed else None))
        return dt.value if timed else None

    def _nztot(self):
        """stored elements of the handle (fixed at creation: read once)"""
        if getattr(self, "_nztot_cached", None) is None:
            self._nztot_cached = self.info()["nztot"]
        return self._nztot_cached

    def sddmm(self, X, Y, G_out, k, accumulate=False, ldx=None, ldy=None, timed=False, stream=None):
        """G (+)= (X * Y^T) sampled on the stored blocks (sparta_vbs_sddmm), device tensors: X rows x k and Y cols x k, column-major (ldx, ldy),
        in the handle's B dtype; G_out float32 with >= nztot elements, in the mab layout of the handle.  With X = dC and Y = B of C = A * B,
        G is the gradient of A's stored values.  Stream-ordered on torch's current stream.  Returns kernel ms if timed else None."""
        import torch
        want = {_lib.F32: torch.float32, _lib.F16: torch.float16, _lib.BF16: torch.bfloat16}[self.dtype]
        if not (X.is_cuda and Y.is_cuda and G_out.is_cuda and X.dtype == want and Y.dtype == want and G_out.dtype == torch.float32):
            raise ValueError("X and Y must be %s tensors and G a float32 tensor, all on the GPU" % want)
        if X.device.index != self.device or Y.device.index != self.device or G_out.device.index != self.device:
            raise ValueError("X, Y and G must live on device %d" % self.device)
        k = int(k)
        if k <= 0:
            raise ValueError("k must be > 0")
        ldx = self.rows if ldx is None else int(ldx)
        ldy = self.cols if ldy is None else int(ldy)
        nztot = self._nztot()
        if (X.numel() < ldx * (k - 1) + self.rows or Y.numel() < ldy * (k - 1) + self.cols or G_out.numel() < nztot
                or not X.is_contiguous() or not Y.is_contiguous() or not G_out.is_contiguous()):
            raise ValueError("X, Y or G too small / not contiguous for the stated leading dimensions")
        st = torch.cuda.current_stream(self.device).cuda_stream if stream is None else stream
        dt = C.c_float(0)
        check(lib.sparta_vbs_sddmm(self.h, C.c_void_p(X.data_ptr()), ldx, C.c_void_p(Y.data_ptr()), ldy, k,
                                   C.cast(C.c_void_p(G_out.data_ptr()), _f32p), int(bool(accumulate)), _lib.PTR_DEVICE, C.c_void_p(st),
                                   C.byref(dt) if timed else None))
        return dt.value if timed else None

    @property
    def updatable(self):
        """was the handle created with updatable=True (sparta_vbs_flags)?"""
        f = C.c_int32(0)
        check(lib.sparta_vbs_flags(self.h, C.byref(f)))
        return bool(f.value & _lib.CREATE_UPDATABLE)

    @property
    def transposable(self):
        """was the handle created with transposable=True (sparta_vbs_flags)?"""
        f = C.c_int32(0)
        check(lib.sparta_vbs_flags(self.h, C.byref(f)))
        return bool(f.value & _lib.CREATE_TRANSPOSE)

    def spmm_t(self, X, Ct_out, n_cols, accumulate=False, ldx=None, ldo=None, timed=False, stream=None):
        """Ct (+)= A^T * X on the stored blocks (sparta_vbs_spmm_t), device tensors: X rows x n_cols, column-major (ldx), in the handle's B dtype;
        Ct_out cols x n_cols, column-major (ldo), float32.  With X = dC of C = A * B, Ct is the gradient of B.  Needs transposable=True.
        Stream-ordered on torch's current stream.  Returns kernel ms if timed else None."""
        import torch
        want = {_lib.F32: torch.float32, _lib.F16: torch.float16, _lib.BF16: torch.bfloat16}[self.dtype]
        if not (X.is_cuda and Ct_out.is_cuda and X.dtype == want and Ct_out.dtype == torch.float32):
            raise ValueError("X must be a %s tensor and Ct a float32 tensor, both on the GPU" % want)
        if X.device.index != self.device or Ct_out.device.index != self.device:
            raise ValueError("X and Ct must live on device %d" % self.device)
        n_cols = int(n_cols)
        if n_cols <= 0:
            raise ValueError("n_cols must be > 0")
        ldx = self.rows if ldx is None else int(ldx)
        ldo = self.cols if ldo is None else int(ldo)
        if (X.numel() < ldx * (n_cols - 1) + self.rows or Ct_out.numel() < ldo * (n_cols - 1) + self.cols
                or not X.is_contiguous() or not Ct_out.is_contiguous()):
            raise ValueError("X or Ct too small / not contiguous for the stated leading dimensions")
        st = torch.cuda.current_stream(self.device).cuda_stream if stream is None else stream
        dt = C.c_float(0)
        check(lib.sparta_vbs_spmm_t(self.h, C.c_void_p(X.data_ptr()), ldx, n_cols, C.cast(C.c_void_p(Ct_out.data_ptr()), _f32p), ldo,
                                    int(bool(accumulate)), _lib.PTR_DEVICE, C.c_void_p(st), C.byref(dt) if timed else None))
        return dt.value if timed else None

    def spmm_t_host(self, X, n_cols, Ct_out, accumulate=True):
        """spmm_t with host buffers (numpy, fp32; X rounded on the device for 16-bit handles): X rows x n_cols, column-major (ld = rows);
        Ct_out a contiguous float32 array of >= cols * n_cols elements (ld = cols), written in place.  Returns kernel ms."""
        X = np.ascontiguousarray(X, np.float32).reshape(-1)
        if not (isinstance(Ct_out, np.ndarray) and Ct_out.dtype == np.float32 and Ct_out.flags.c_contiguous):
            raise ValueError("Ct must be a contiguous float32 numpy array (it is written in place)")
        n_cols = int(n_cols)
        if n_cols <= 0:
            raise ValueError("n_cols must be > 0")
        if X.size < self.rows * n_cols or Ct_out.size < self.cols * n_cols:
            raise ValueError("X or Ct too small")
        dt = C.c_float(0)
        check(lib.sparta_vbs_spmm_t(self.h, X.ctypes.data_as(C.c_void_p), self.rows, n_cols, Ct_out.ctypes.data_as(_f32p), self.cols,
                                    int(bool(accumulate)), _lib.PTR_HOST, None, C.byref(dt)))
        return dt.value

    def set_values(self, mab, timed=False, stream=None):
        """sparta_vbs_set_values, device tensor: new values for the stored blocks (same pattern), a contiguous float32 tensor of nztot elements
        on this device in the layout of VBR.mab (= G of sddmm; for a range handle the slice of its block-rows).  Stream-ordered on torch's current
        stream; every later product behaves as if the handle had been created from these values.  Needs updatable=True.  Returns kernel ms if timed."""
        import torch
        if not (mab.is_cuda and mab.dtype == torch.float32 and mab.device.index == self.device and mab.is_contiguous()):
            raise ValueError("mab must be a contiguous float32 tensor on device %d" % self.device)
        if mab.numel() != self._nztot():
            raise ValueError("mab must hold nztot = %d elements" % self._nztot())
        st = torch.cuda.current_stream(self.device).cuda_stream if stream is None else stream
        dt = C.c_float(0)
        self._values_replaced()
        check(lib.sparta_vbs_set_values(self.h, C.cast(C.c_void_p(mab.data_ptr()), _f32p), _lib.PTR_DEVICE, C.c_void_p(st),
                                        C.byref(dt) if timed else None))
        return dt.value if timed else None

    def sgd_step(self, values, grad, momentum_buf=None, lr=None, momentum=0.0, weight_decay=0.0, grad_scale=1.0, timed=False, stream=None, ctl=None):
        """sparta_vbs_sgd_step, device tensors: one SGD step on `values` (the float32 master copy, updated in place) with the gradient `grad` (what sddmm
        writes) and, when momentum != 0, the buffer `momentum_buf` (updated in place; zeros before the first step) -- torch.optim.SGD with dampening 0 and no
        Nesterov, grad first multiplied by grad_scale -- and the handle's images written from the new values in the same pass: afterwards the handle behaves
        as after set_values(values).  All three: contiguous float32 tensors of nztot elements on this device, in the layout of VBR.mab.  Stream-ordered on
        torch's current stream.  The version counter of `values` is bumped (a backward of a forward taken before the step raises, as after any in-place
        change) and the handle records the new version, so that the next vbs_linear forward with the same tensor skips set_values.  Needs updatable=True.
        ctl: a GradCtl (or its tensor) after finish() -- sparta_vbs_sgd_step_ctl: the gradient is also multiplied by the record's coef, and a record that says
        skip leaves values and momentum_buf as they are (the handle is written from values all the same); both are read on the device.
        Returns kernel ms if timed else None."""
        import torch
        if lr is None:
            raise ValueError("lr is required")
        ops = [("values", values), ("grad", grad)] + ([("momentum_buf", momentum_buf)] if momentum_buf is not None else [])
        for name, t in ops:
            if not (t.is_cuda and t.dtype == torch.float32 and t.device.index == self.device and t.is_contiguous()):
                raise ValueError("%s must be a contiguous float32 tensor on device %d" % (name, self.device))
            if t.numel() != self._nztot():
                raise ValueError("%s must hold nztot = %d elements" % (name, self._nztot()))
        st = torch.cuda.current_stream(self.device).cuda_stream if stream is None else stream
        cfg = _lib.SgdCfg(float(lr), float(momentum), float(weight_decay), float(grad_scale))
        dt = C.c_float(0)
        self._values_replaced()
        R = _ctl_ptr(ctl, self.device)
        check(lib.sparta_vbs_sgd_step_ctl(self.h, C.cast(C.c_void_p(values.data_ptr()), _f32p), C.cast(C.c_void_p(grad.data_ptr()), _f32p),
                                          None if momentum_buf is None else C.cast(C.c_void_p(momentum_buf.data_ptr()), _f32p), C.byref(cfg), R,
                                          C.c_void_p(st), C.byref(dt) if timed else None))
        # the kernels wrote through the raw pointers: tell autograd, then note that the handle holds exactly this version
        bump = getattr(torch.autograd.graph, "increment_version", None)
        for t in (values,) + (() if momentum_buf is None else (momentum_buf,)):
            if bump is not None:
                bump(t)
            else:
                with torch.no_grad():
                    t.add_(0)
        if torch.cuda.is_current_stream_capturing():
            self._autograd_captured = True          # (as a captured forward: replays change the handle's values without passing through Python)
        if not self._autograd_captured:
            self._autograd_values = (values, values._version)
        return dt.value if timed else None

    def adam_step(self, values, grad, exp_avg, exp_avg_sq, state, lr=None, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=True, grad_scale=1.0,
                  timed=False, stream=None, ctl=None):
        """sparta_vbs_adam_step, device tensors: one AdamW (decoupled=True) / Adam with L2 weight decay (decoupled=False) step on `values` (the float32
        master copy, updated in place) with the gradient `grad`, the moments `exp_avg` and `exp_avg_sq` (updated in place; zeros before the first step) and
        `state`, a contiguous tensor of 8 int32 or float32 words on this device that holds the step count and the bias corrections (zeros: a fresh optimizer;
        advanced on the device, so a captured step replays correctly) -- torch.optim.AdamW / Adam without amsgrad and maximize, grad first multiplied by
        grad_scale -- and the handle's images written from the new values in the same pass: afterwards the handle behaves as after set_values(values).  The
        four operands: contiguous float32 tensors of nztot elements on this device, in the layout of VBR.mab.  Stream-ordered on torch's current stream.  lr
        and the other hyper-parameters are baked into a capture.  The version counters of `values`, `exp_avg` and `exp_avg_sq` are bumped and the handle
        records the new version of `values`, so that the next vbs_linear forward with the same tensor skips set_values.  Needs updatable=True.  ctl: as for
        sgd_step (sparta_vbs_adam_step_ctl); a skipped step does not advance the step count either.  Returns kernel ms if timed else None."""
        import torch
        if lr is None:
            raise ValueError("lr is required")
        for name, t in (("values", values), ("grad", grad), ("exp_avg", exp_avg), ("exp_avg_sq", exp_avg_sq)):
            if t is None or not (t.is_cuda and t.dtype == torch.float32 and t.device.index == self.device and t.is_contiguous()):
                raise ValueError("%s must be a contiguous float32 tensor on device %d" % (name, self.device))
            if t.numel() != self._nztot():
                raise ValueError("%s must hold nztot = %d elements" % (name, self._nztot()))
        if state is None or not (state.is_cuda and state.dtype in (torch.int32, torch.float32) and state.device.index == self.device
                                 and state.is_contiguous() and state.numel() == 8):
            raise ValueError("state must be a contiguous tensor of 8 int32 or float32 words on device %d" % self.device)
        st = torch.cuda.current_stream(self.device).cuda_stream if stream is None else stream
        cfg = _lib.AdamCfg(float(lr), float(betas[0]), float(betas[1]), float(eps), float(weight_decay), float(grad_scale), int(bool(decoupled)), 0)
        dt = C.c_float(0)
        self._values_replaced()
        R = _ctl_ptr(ctl, self.device)
        check(lib.sparta_vbs_adam_step_ctl(self.h, *(C.cast(C.c_void_p(t.data_ptr()), _f32p) for t in (values, grad, exp_avg, exp_avg_sq)),
                                           C.c_void_p(state.data_ptr()), C.byref(cfg), R, C.c_void_p(st), C.byref(dt) if timed else None))
        # the kernels wrote through the raw pointers: tell autograd, then note that the handle holds exactly this version
        bump = getattr(torch.autograd.graph, "increment_version", None)
        for t in (values, exp_avg, exp_avg_sq):
            if bump is not None:
                bump(t)
            else:
                with torch.no_grad():
                    t.add_(0)
        if torch.cuda.is_current_stream_capturing():
            self._autograd_captured = True          # (as a captured forward: replays change the handle's values without passing through Python)
        if not self._autograd_captured:
            self._autograd_values = (values, values._version)
        return dt.value if timed else None

    def step_info(self):
        """sparta_vbs_step_info: {"fused": 1 the last sgd_step / adam_step did its arithmetic inside an image kernel / 0 it ran the elementwise kernel and then
        the set_values launches / -1 no step yet, "launches": kernel launches of that step (an Adam step counts its tick)}; ["live"]: 1 if that step
        skipped dead blocks (set_live_steps), else 0 -- a later word, see _Info"""
        out = (C.c_int64 * 4)()
        check(lib.sparta_vbs_step_info(self.h, out))
        return _Info({"fused": int(out[0]), "launches": int(out[1])}, {"live": int(out[2])})

    @property
    def n_blocks(self):
        """stored blocks of the handle (sparta_vbs_block_count), those of block-rows of height 0 included: the length of block_ssq's result and of keep"""
        if getattr(self, "_n_blocks_cached", None) is None:
            n = C.c_int64(0)
            check(lib.sparta_vbs_block_count(self.h, C.byref(n)))
            self._n_blocks_cached = int(n.value)
        return self._n_blocks_cached

    def _prune_operand(self, name, t):
        import torch
        if not (t.is_cuda and t.dtype == torch.float32 and t.device.index == self.device and t.is_contiguous()):
            raise ValueError("%s must be a contiguous float32 tensor on device %d" % (name, self.device))
        if t.numel() != self._nztot():
            raise ValueError("%s must hold nztot = %d elements" % (name, self._nztot()))
        return C.cast(C.c_void_p(t.data_ptr() if t.numel() else None), _f32p)

    def block_ssq(self, values, out=None, timed=False, stream=None):
        """sparta_vbs_block_ssq, device tensors: per stored block (mab order: VBR.block_table) the float64 sum of the squares of those of its elements
        of `values` that lie inside the matrix.  values: a contiguous float32 tensor of nztot elements on this device in the layout of VBR.mab (weights,
        a gradient, ...).  out: a contiguous float64 tensor of n_blocks elements on this device, or None (allocated).  Stream-ordered on torch's
        current stream; one kernel launch after the first call on the handle.  Returns out, or (out, kernel ms) if timed."""
        import torch
        W = self._prune_operand("values", values)
        n = self.n_blocks
        if out is None:
            out = torch.empty(n, dtype=torch.float64, device=values.device)
        elif not (out.is_cuda and out.dtype == torch.float64 and out.device.index == self.device and out.is_contiguous() and out.numel() == n):
            raise ValueError("out must be a contiguous float64 tensor of n_blocks = %d elements on device %d" % (n, self.device))
        st = torch.cuda.current_stream(self.device).cuda_stream if stream is None else stream
        dt = C.c_float(0)
        check(lib.sparta_vbs_block_ssq(self.h, W, C.cast(C.c_void_p(out.data_ptr() if n else None), C.POINTER(C.c_double)), C.c_void_p(st),
                                       C.byref(dt) if timed else None))
        return (out, dt.value) if timed else out

    def sddmm_block_ssq(self, X, Y, k, sel=None, out=None, ldx=None, ldy=None, timed=False, stream=None):
        """sparta_vbs_sddmm_block_ssq, device tensors: per stored block the float64 sum of the squares of what sddmm(X, Y, accumulate=False) would store for
        it on a handle without a live set -- block_ssq of that gradient -- without writing the gradient.  X, Y, k, ldx, ldy: as for sddmm.  sel: a contiguous
        uint8 or bool tensor of n_blocks elements on this device (numbered as for mask_blocks), or None = every block; a block with sel[b] == 0 scores +0.0
        and the operands are not read on its behalf.  out: a contiguous float64 tensor of n_blocks elements on this device, or None (allocated).  The live
        set of the handle, installed or not, plays no part and is not changed.  Stream-ordered on torch's current stream; launches only after the first
        call on the handle (capturable from then on; a replay reads X, Y and sel again).  Returns out, or (out, kernel ms) if timed."""
        import torch
        want = {_lib.F32: torch.float32, _lib.F16: torch.float16, _lib.BF16: torch.bfloat16}[self.dtype]
        if not (X.is_cuda and Y.is_cuda and X.dtype == want and Y.dtype == want):
            raise ValueError("X and Y must be %s tensors on the GPU" % want)
        if X.device.index != self.device or Y.device.index != self.device:
            raise ValueError("X and Y must live on device %d" % self.device)
        k = int(k)
        if k <= 0:
            raise ValueError("k must be > 0")
        ldx = self.rows if ldx is None else int(ldx)
        ldy = self.cols if ldy is None else int(ldy)
        if (X.numel() < ldx * (k - 1) + self.rows or Y.numel() < ldy * (k - 1) + self.cols or not X.is_contiguous() or not Y.is_contiguous()):
            raise ValueError("X or Y too small / not contiguous for the stated leading dimensions")
        n = self.n_blocks
        if sel is not None and not (sel.is_cuda and sel.dtype in (torch.uint8, torch.bool) and sel.device.index == self.device and sel.is_contiguous()
                                    and sel.numel() == n):
            raise ValueError("sel must be a contiguous uint8 or bool tensor of n_blocks = %d elements on device %d" % (n, self.device))
        if out is None:
            out = torch.empty(n, dtype=torch.float64, device=X.device)
        elif not (out.is_cuda and out.dtype == torch.float64 and out.device.index == self.device and out.is_contiguous() and out.numel() == n):
            raise ValueError("out must be a contiguous float64 tensor of n_blocks = %d elements on device %d" % (n, self.device))
        st = torch.cuda.current_stream(self.device).cuda_stream if stream is None else stream
        dt = C.c_float(0)
        sp = C.cast(C.c_void_p(sel.data_ptr() if sel is not None and n else None), C.POINTER(C.c_uint8))
        check(lib.sparta_vbs_sddmm_block_ssq(self.h, C.c_void_p(X.data_ptr()), ldx, C.c_void_p(Y.data_ptr()), ldy, k, sp,
                                             C.cast(C.c_void_p(out.data_ptr() if n else None), C.POINTER(C.c_double)), C.c_void_p(st),
                                             C.byref(dt) if timed else None))
        return (out, dt.value) if timed else out

    def mask_blocks(self, keep, *tensors, timed=False, stream=None):
        """sparta_vbs_mask_blocks, device tensors: every block b with keep[b] == 0 stored as +0.0 -- all its elements, the positions past cols included
        -- in each of `tensors` (contiguous float32 tensors of nztot elements on this device in the layout of VBR.mab, updated in place; they must not
        overlap); the other blocks are not touched.  keep: a contiguous uint8 or bool tensor of n_blocks elements on this device.  One launch per
        group of up to four tensors.  The handle's own images are NOT changed and the handle does not learn which tensor holds its values: follow
        with set_values (or a step) to make it multiply with the masked values.  The version counters of the tensors are bumped.  Stream-ordered on
        torch's current stream.  Returns kernel ms if timed else None."""
        import torch
        if not tensors:
            raise ValueError("mask_blocks needs at least one tensor")
        n = self.n_blocks
        if not (keep.is_cuda and keep.dtype in (torch.uint8, torch.bool) and keep.device.index == self.device and keep.is_contiguous() and keep.numel() == n):
            raise ValueError("keep must be a contiguous uint8 or bool tensor of n_blocks = %d elements on device %d" % (n, self.device))
        ptrs = [self._prune_operand("tensor %d" % i, t) for i, t in enumerate(tensors)]
        st = torch.cuda.current_stream(self.device).cuda_stream if stream is None else stream
        kp = C.cast(C.c_void_p(keep.data_ptr() if n else None), C.POINTER(C.c_uint8))
        total = 0.0
        for g in range(0, len(ptrs), 4):
            grp = ptrs[g:g + 4] + [None] * (4 - len(ptrs[g:g + 4]))
            dt = C.c_float(0)
            check(lib.sparta_vbs_mask_blocks(self.h, kp, *grp, C.c_void_p(st), C.byref(dt) if timed else None))
            total += dt.value
        bump = getattr(torch.autograd.graph, "increment_version", None)
        for t in tensors:
            if bump is not None:
                bump(t)
            else:
                with torch.no_grad():
                    t.add_(0)
        return total if timed else None

    def set_live_blocks(self, keep, stream=None):
        """sparta_vbs_set_live_blocks: from now on sddmm and spmm_t of this handle skip every block b with keep[b] == 0 -- its gradient is +0.0 (accumulate=
        False) or left as it is (True), and it adds nothing to spmm_t; the operands are not read on its behalf.  keep: a contiguous uint8 or bool tensor of
        n_blocks elements on this device, numbered as for mask_blocks; the handle takes a snapshot in stream order (torch's current stream).  keep=None
        removes the live set.  Nothing else changes: the forward products, set_values and the steps ignore it, so the values of the dead blocks must be
        zero for forward and backward to agree (BlockPruner does that).  Launches only after the first call on the handle (capturable from then on)."""
        if keep is None:
            check(lib.sparta_vbs_set_live_blocks(self.h, None, None))
            return
        import torch
        n = self.n_blocks
        if not (keep.is_cuda and keep.dtype in (torch.uint8, torch.bool) and keep.device.index == self.device and keep.is_contiguous() and keep.numel() == n):
            raise ValueError("keep must be a contiguous uint8 or bool tensor of n_blocks = %d elements on device %d" % (n, self.device))
        st = torch.cuda.current_stream(self.device).cuda_stream if stream is None else stream
        if n == 0:                                             # (no byte to point at: an all-live set of no blocks is no live set)
            check(lib.sparta_vbs_set_live_blocks(self.h, None, None))
            return
        check(lib.sparta_vbs_set_live_blocks(self.h, C.cast(C.c_void_p(keep.data_ptr()), C.POINTER(C.c_uint8)), C.c_void_p(st)))

    def set_live_steps(self, on, stream=None):
        """sparta_vbs_set_live_steps: with on=True and a live set installed (set_live_blocks) sgd_step / adam_step, plain and under a GradCtl, skip the dead
        blocks: their G, M, V are neither read nor written, W is not written (it must hold +0.0 there, as mask_blocks leaves it) and the images get +0.0.
        Live blocks get the bits of the plain step.  Off by default; without a live set the switch does nothing.  The first enabling call builds helper
        arrays and cannot be captured; later calls, and set_live_blocks with the switch on, are launches only (torch's current stream).  Nothing to gain
        on an unpruned set.  step_info()["live"] says what the last step did."""
        if not on:
            check(lib.sparta_vbs_set_live_steps(self.h, 0, None))
            return
        check(lib.sparta_vbs_set_live_steps(self.h, 1, self._live_stream(stream)))

    def set_live_forward(self, on, stream=None):
        """sparta_vbs_set_live_forward: with on=True and a live set installed (set_live_blocks) the 16-bit forward product walks the steps of live blocks only:
        a dead block adds nothing to C whatever the handle holds for it, and neither its values nor the rows of B are read on its behalf.  On values whose
        dead blocks are zero (what BlockPruner leaves) C is the plain product, the sign of a zero aside.  Needs updatable=True.  Handles without the live form
        (fp32, a hub plan, two stream images, block widths that are no multiple of 32) accept the switch and keep their kernels: live_forward_info() says
        which.  Off by default; without a live set the switch does nothing.  The first enabling call builds helper arrays and cannot be captured; later
        calls, and set_live_blocks from then on, are launches only (torch's current stream).  Refused while set_forward_a8 is on: set_a8_live is the switch
        for the product on the fp8 image."""
        if not on:
            check(lib.sparta_vbs_set_live_forward(self.h, 0, None))
            return
        check(lib.sparta_vbs_set_live_forward(self.h, 1, self._live_stream(stream)))

    def live_forward_info(self, stream=None):
        """sparta_vbs_live_forward_info (synchronises when a live set is installed): {"switch", "capable" (the stream image with the live form: 0 none, 1 the <= 32-row tiles, 2 the 64-row / pair tiles), "form_one_tile", "form_pair" (what the last 16-bit
        product ran on each stream image: 0 none yet, 1 the plain kernels, 2 the live kernels), "steps", "kept_steps", "split_tiles", "ranges"}"""
        a = np.zeros(8, np.int64)
        check(lib.sparta_vbs_live_forward_info(self.h, a.ctypes.data_as(_i64p), self._live_stream(stream)))
        keys = ["switch", "capable", "form_one_tile", "form_pair", "steps", "kept_steps", "split_tiles", "ranges"]
        return {k: int(a[i]) for i, k in enumerate(keys)}

    def live_forward_lists(self, stream=None):
        """sparta_vbs_live_forward_lists_get (synchronises; for tests and records): {"steps": the plain records of the stream image with the live form (a
        structured array, host.STEP_DTYPE), "ranges": int32 [ranges][2], "live": uint8 [steps][2] (rows 0..31 / 32..63 of every step's slice), "pair": whether
        the image holds 64-row / pair tiles, "steps_live", "ranges_live": what the live kernels walk}.  host.live_forward_compact(steps, ranges, pair, live)
        is the same rule on the host."""
        from .host import STEP_DTYPE
        fi = self.live_forward_info(stream)
        n, nr = fi["steps"], fi["ranges"]
        out = {"steps": np.zeros(n, STEP_DTYPE), "ranges": np.zeros((nr, 2), np.int32), "live": np.zeros((n, 2), np.uint8),
               "steps_live": np.zeros(n, STEP_DTYPE), "ranges_live": np.zeros((nr, 2), np.int32)}
        i32p, u8p = C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
        check(lib.sparta_vbs_live_forward_lists_get(self.h, out["steps"].ctypes.data_as(C.c_void_p), out["ranges"].ctypes.data_as(i32p), out["live"].ctypes.data_as(u8p),
                                                    out["steps_live"].ctypes.data_as(C.c_void_p), out["ranges_live"].ctypes.data_as(i32p), self._live_stream(stream)))
        out["pair"] = fi["capable"] == 2
        return out

    def set_forward_a8(self, on, values=None, stream=None):
        """sparta_vbs_set_forward_a8: with on=True the 16-bit forward product multiplies with an fp8 (OCP e4m3) image of the weights -- one byte per element, one
        power-of-two scale per group of <= 32 rows x 32 / 64 values of a stored block, widened to the handle's 16-bit type in registers -- instead of the 16-bit
        image.  spmm_t, sddmm, the steps and everything else keep reading the 16-bit image: under vbs_linear that is quantisation-aware training with a
        straight-through backward.  Needs updatable=True and a 16-bit handle whose one stream image holds every stored element (a8_info()["capable"]); every
        other handle raises SpartaError (unsupported), as does a handle with live forward on.  The image is invalid (the product keeps the 16-bit weights) until
        the next set_values / sgd_step / adam_step, each of which requantises behind itself while the switch is on; values=W is the switch followed by
        set_values(W).  An Inf weight becomes NaN under the switch (e4m3fn has no Inf).  Off by default.  The first enabling call allocates and cannot be
        captured.  set_a8_live is the switch that lets this product skip pruned blocks."""
        if not on:
            check(lib.sparta_vbs_set_forward_a8(self.h, 0, None))
            return
        check(lib.sparta_vbs_set_forward_a8(self.h, 1, self._live_stream(stream)))
        self._values_replaced()                                # (the next vbs_linear forward writes its values, and with them the image)
        if values is not None:
            self.set_values(values, stream=stream)

    def a8_info(self, stream=None):
        """sparta_vbs_a8_info: {"switch", "valid" (the image follows the current values), "capable" (the stream image with the a8 form: 0 none, 1 the <= 32-row
        tiles, 2 the 64-row / pair tiles), "form_one_tile", "form_pair" (what the last 16-bit product ran on each stream image: 0 none yet, 1 the plain
        kernels, 2 live, 3 a8), "groups", "image_bytes", "quantize_launches"}"""
        a = np.zeros(8, np.int64)
        check(lib.sparta_vbs_a8_info(self.h, a.ctypes.data_as(_i64p), self._live_stream(stream)))
        keys = ["switch", "valid", "capable", "form_one_tile", "form_pair", "groups", "image_bytes", "quantize_launches"]
        return {k: int(a[i]) for i, k in enumerate(keys)}

    def set_a8_live(self, on, stream=None):
        """sparta_vbs_set_a8_live: with on=True, the fp8 switch on (set_forward_a8) and a live set installed (set_live_blocks) the product on the fp8 image walks
        the steps of live blocks only: a dead block adds nothing to C whatever W, the codes or the exponents hold for it, and neither its codes nor the rows of
        B are read on its behalf.  C is, bit for bit, the live forward product of a plain handle on the dequantised values.  Needs set_forward_a8 on: SpartaError
        (unsupported) otherwise; set_forward_a8(False) clears this switch too.  Off by default; without a live set the a8 kernels multiply every block.  The first
        enabling call builds the helper arrays of live forward and cannot be captured; later calls, and set_live_blocks and every write of values from then on,
        are launches only (torch's current stream).  a8_info()["form_*"] says 4 when the product took this form."""
        if not on:
            check(lib.sparta_vbs_set_a8_live(self.h, 0, None))
            return
        check(lib.sparta_vbs_set_a8_live(self.h, 1, self._live_stream(stream)))

    def a8_live_info(self, stream=None):
        """sparta_vbs_a8_live_info (synchronises when a live set is installed): {"switch", "active" (the fp8 switch on and its image valid, this switch on, a live
        set installed), "capable" (the stream image with the form: 0 none, 1 the <= 32-row tiles, 2 the 64-row / pair tiles), "steps", "kept_steps",
        "scale_launches" (launches of the scale-placement kernel so far)}"""
        a = np.zeros(8, np.int64)
        check(lib.sparta_vbs_a8_live_info(self.h, a.ctypes.data_as(_i64p), self._live_stream(stream)))
        keys = ["switch", "active", "capable", "steps", "kept_steps", "scale_launches"]
        return {k: int(a[i]) for i, k in enumerate(keys)}

    def a8_get(self, stream=None):
        """sparta_vbs_a8_get (synchronises; for tests and records): (codes uint8, exps int32, group int32), nztot elements each in the layout of VBR.mab -- the
        e4m3fn code of every stored element, the exponent of its group (its dequantised value is the code times 2^exp) and the number of its group."""
        n = self._nztot()
        codes, exps, group = np.zeros(n, np.uint8), np.zeros(n, np.int32), np.full(n, -1, np.int32)      # (an element no group covers would keep its -1)
        i32p, u8p = C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
        check(lib.sparta_vbs_a8_get(self.h, codes.ctypes.data_as(u8p), exps.ctypes.data_as(i32p), group.ctypes.data_as(i32p), self._live_stream(stream)))
        return codes, exps, group

    def _live_stream(self, stream):
        import torch
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream if stream is None else stream)

    def live_info(self, stream=None):
        """sparta_vbs_live_info (synchronises): {"installed", "n_blocks", "live_blocks", "sd_groups", "live_sd_groups", "t_entries", "live_t_entries"};
        ["live_steps"]: the switch of set_live_steps -- a later word, see _Info"""
        a = np.zeros(8, np.int64)
        check(lib.sparta_vbs_live_info(self.h, a.ctypes.data_as(_i64p), self._live_stream(stream)))
        keys = ["installed", "n_blocks", "live_blocks", "sd_groups", "live_sd_groups", "t_entries", "live_t_entries"]
        return _Info({k: int(a[i]) for i, k in enumerate(keys)}, {"live_steps": int(a[7])})

    def live_lists(self, stream=None):
        """sparta_vbs_live_lists_get (synchronises; for tests): the compacted lists the kernels walk, as VBR.live_lists returns them for the same keep --
        {"sd_groups", "sd_count", "t_blocks", "t_count"}, int32 arrays; the last two are empty on a handle made without transposable=True"""
        li, info = self.live_info(stream), self.info()
        if not li["installed"]:
            raise ValueError("no live set is installed")
        i32p = C.POINTER(C.c_int32)
        block_cols = (info["cols"] - 1) // info["block_col_size"] + 1
        out = {"sd_groups": np.zeros(li["sd_groups"], np.int32), "sd_count": np.zeros(info["block_rows"], np.int32),
               "t_blocks": np.zeros(li["t_entries"], np.int32), "t_count": np.zeros(block_cols if self.transposable else 0, np.int32)}
        check(lib.sparta_vbs_live_lists_get(self.h, *(out[k].ctypes.data_as(i32p) if out[k].size else None for k in ("sd_groups", "sd_count", "t_blocks", "t_count")),
                                            self._live_stream(stream)))
        return out

    def move_blocks(self, src, map, *pairs, timed=False, stream=None):
        """sparta_vbs_move_blocks with this handle as the destination: tensors moved from the mab layout of `src` (another DeviceVBS on this device) to this
        handle's.  map: int32, one entry per block of THIS handle -- the block of src it receives, or -1 for a new block, which becomes +0.0 (VBR.repattern
        returns such a map; any map whose mapped blocks agree in size will do).  pairs: (src_tensor, dst_tensor), contiguous float32 tensors on this device of
        nztot(src) and nztot(this) elements; the destinations are overwritten completely (they may be torch.empty) and must overlap nothing.  Blocks travel bit
        for bit.  One launch per group of up to four pairs.  The handles' own images are NOT changed: follow with set_values.  A rare operation: it
        synchronises the stream (torch's current one) and cannot be captured.  Returns kernel ms if timed else None."""
        import torch
        if not isinstance(src, DeviceVBS) or src.device != self.device:
            raise ValueError("src must be a DeviceVBS on device %d" % self.device)
        bmap = np.ascontiguousarray(map, np.int32).reshape(-1)
        if bmap.size != self.n_blocks:
            raise ValueError("map must hold n_blocks = %d elements" % self.n_blocks)
        ptrs = []
        for i, (s, d) in enumerate(pairs):
            sp, dp = src._prune_operand("source tensor %d" % i, s), self._prune_operand("destination tensor %d" % i, d)
            if d.numel() == 0:                                 # (nothing to write: an empty tensor has no address to give, and a half-NULL pair is refused)
                continue
            if s.numel() == 0:                                 # (every block is new and nothing is read: any valid address stands for the empty source)
                keep_alive = torch.empty(1, dtype=torch.float32, device=d.device)
                sp = C.cast(C.c_void_p(keep_alive.data_ptr()), _f32p)
            ptrs.append((sp, dp))
        st = torch.cuda.current_stream(self.device).cuda_stream if stream is None else stream
        mp = bmap.ctypes.data_as(C.POINTER(C.c_int32)) if bmap.size else None
        total = 0.0
        for g in range(0, max(len(ptrs), 1), 4):
            grp = [p for pair in ptrs[g:g + 4] for p in pair] + [None] * (8 - 2 * len(ptrs[g:g + 4]))
            dt = C.c_float(0)
            check(lib.sparta_vbs_move_blocks(self.h, src.h, mp, *grp, C.c_void_p(st), C.byref(dt) if timed else None))
            total += dt.value
        return total if timed else None

    def _dense_operand(self, D):
        layout, ldd, dt = _dense_layout(D)
        if D.device.index != self.device:
            raise ValueError("D must live on device %d" % self.device)
        if tuple(D.shape) != (self.rows, self.cols):
            raise ValueError("D must be %d x %d (the rows of the handle's block-rows x cols)" % (self.rows, self.cols))
        return layout, ldd, dt

    def gather_dense(self, D, out=None, timed=False, stream=None):
        """sparta_vbs_gather_dense, device tensors: the dense matrix D sampled into the mab layout of the handle -- values[off + q * h + i] = D[r0 + i, jb * w
        + q] for every stored block; the stored positions past cols get +0.0; nothing of D outside the stored blocks is read.  D: a 2-D float32, float16 or
        bfloat16 tensor on this device of the handle's rows x cols (a range handle: the rows of its block-rows), independent of the handle's own dtype; the
        layout and the leading dimension are taken from its strides, one of which must be 1 (row-major: nn.Linear.weight as it is; column-major: its .t())
        -- anything else raises ValueError, nothing is copied silently.  fp32 and bf16 values arrive bit for bit, fp16 exactly.  out: a contiguous float32
        tensor of nztot elements on this device, or None (allocated); every element is written.  The handle's images are NOT changed: follow with
        set_values.  Stream-ordered on torch's current stream; launches only after the first gather_dense / scatter_dense on the handle (capturable from
        then on).  Returns out, or (out, kernel ms) if timed."""
        import torch
        layout, ldd, dt_code = self._dense_operand(D)
        n = self._nztot()
        if out is None:
            out = torch.empty(n, dtype=torch.float32, device=D.device)
        T = self._prune_operand("out", out)
        st = torch.cuda.current_stream(self.device).cuda_stream if stream is None else stream
        dt = C.c_float(0)
        check(lib.sparta_vbs_gather_dense(self.h, C.c_void_p(D.data_ptr() if D.numel() else None), ldd, layout, dt_code, C.cast(T, C.c_void_p), C.c_void_p(st),
                                          C.byref(dt) if timed else None))
        return (out, dt.value) if timed else out

    def scatter_dense(self, values, D, fill=True, timed=False, stream=None):
        """sparta_vbs_scatter_dense, device tensors: the inverse of gather_dense, D[r0 + i, jb * w + q] = values[off + q * h + i] for every stored block (the
        stored positions past cols are not read), written in place into D (as for gather_dense: float32, float16 or bfloat16, one stride 1; a 16-bit D gets
        the handle-creation rounding, nearest even).  fill=True: the rest of the rows x cols region becomes +0, so that D is the dense form of the sparse
        matrix; fill=False: the rest keeps its bits.  Padding between rows (columns) of a strided D is never written.  A handle that stores a block column
        twice in one block-row is refused.  The version counter of D is bumped.  Stream-ordered on torch's current stream; capturable after the first
        gather_dense / scatter_dense on the handle.  Returns kernel ms if timed else None."""
        import torch
        layout, ldd, dt_code = self._dense_operand(D)
        T = self._prune_operand("values", values.detach())
        st = torch.cuda.current_stream(self.device).cuda_stream if stream is None else stream
        dt = C.c_float(0)
        check(lib.sparta_vbs_scatter_dense(self.h, C.cast(T, C.c_void_p), C.c_void_p(D.data_ptr() if D.numel() else None), ldd, layout, dt_code, int(bool(fill)),
                                           C.c_void_p(st), C.byref(dt) if timed else None))
        bump = getattr(torch.autograd.graph, "increment_version", None)
        if bump is not None:
            bump(D)
        else:
            with torch.no_grad():
                D.add_(0)
        return dt.value if timed else None

    def to_dense(self, values, dtype=None, row_major=True):
        """a fresh rows x cols tensor (dtype: torch.float32 by default, float16 or bfloat16) holding `values` in the stored blocks and +0 elsewhere:
        scatter_dense with fill into an allocation of its own.  row_major=False returns the same matrix with column-major strides."""
        import torch
        dtype = torch.float32 if dtype is None else dtype
        if row_major:
            D = torch.empty((self.rows, self.cols), dtype=dtype, device=values.device)
        else:
            D = torch.empty((self.cols, self.rows), dtype=dtype, device=values.device).t()
        self.scatter_dense(values, D, fill=True)
        return D

    def set_values_host(self, mab):
        """set_values with a host array (numpy, fp32, nztot elements), staged through scratch of the handle.  Returns kernel ms."""
        mab = np.ascontiguousarray(mab, np.float32).reshape(-1)
        if mab.size != self._nztot():
            raise ValueError("mab must hold nztot = %d elements" % self._nztot())
        dt = C.c_float(0)
        self._values_replaced()
        check(lib.sparta_vbs_set_values(self.h, mab.ctypes.data_as(_f32p), _lib.PTR_HOST, None, C.byref(dt)))
        return dt.value

    def sddmm_host(self, X, Y, k, G_out, accumulate=True):
        """sddmm with host buffers (numpy, fp32; rounded on the device for 16-bit handles): X rows x k, Y cols x k, column-major;
        G_out a contiguous float32 array of >= nztot elements, written in place.  Returns kernel ms."""
        X = np.ascontiguousarray(X, np.float32).reshape(-1)
        Y = np.ascontiguousarray(Y, np.float32).reshape(-1)
        if not (isinstance(G_out, np.ndarray) and G_out.dtype == np.float32 and G_out.flags.c_contiguous):
            raise ValueError("G must be a contiguous float32 numpy array (it is written in place)")
        k = int(k)
        if k <= 0:
            raise ValueError("k must be > 0")
        if X.size < self.rows * k or Y.size < self.cols * k or G_out.size < self._nztot():
            raise ValueError("X, Y or G too small")
        dt = C.c_float(0)
        check(lib.sparta_vbs_sddmm(self.h, X.ctypes.data_as(C.c_void_p), self.rows, Y.ctypes.data_as(C.c_void_p), self.cols, k,
                                   G_out.ctypes.data_as(_f32p), int(bool(accumulate)), _lib.PTR_HOST, None, C.byref(dt)))
        return dt.value

    def spmm_gathered(self, B_gathered, shard_rows, C_out, n_cols, accumulate=False, algo=_lib.SPMM_MFMA,
                      c_layout=_lib.COL_MAJOR, shard_stride=None, timed=False, stream=None, shard_ld=None):
        """Multi-GPU entry: B_gathered is the all-gather result (n_shards column-major slabs of shard_rows x n_cols; shard_ld: elements between the columns of a
        slab, default shard_rows -- pad it when shard_rows is a multiple of a large power of two: sparta_vbs_spmm_gathered_ld)."""
        import torch
        want_b = {_lib.F32: torch.float32, _lib.F16: torch.float16, _lib.BF16: torch.bfloat16}[self.dtype]
        if not (B_gathered.is_cuda and C_out.is_cuda and B_gathered.dtype == want_b and C_out.dtype == torch.float32):
            raise ValueError("B_gathered must be a %s tensor and C a float32 tensor, both on the GPU" % want_b)
        if B_gathered.device.index != self.device or C_out.device.index != self.device:
            raise ValueError("B_gathered and C must live on device %d" % self.device)
        shard_ld = shard_rows if shard_ld is None else int(shard_ld)
        shard_stride = shard_ld * n_cols if shard_stride is None else shard_stride
        if B_gathered.numel() < (self.cols // shard_rows - 1) * shard_stride + shard_ld * (n_cols - 1) + shard_rows:
            raise ValueError("B_gathered too small")
        ldc = self.rows if c_layout == _lib.COL_MAJOR else n_cols
        need_c = ldc * (n_cols if c_layout == _lib.COL_MAJOR else self.rows)
        if C_out.numel() < need_c or not B_gathered.is_contiguous() or not C_out.is_contiguous():
            raise ValueError("C too small / B_gathered or C not contiguous")
        st = torch.cuda.current_stream(self.device).cuda_stream if stream is None else stream
        dt = C.c_float(0)
        check(lib.sparta_vbs_spmm_gathered_ld(self.h, C.c_void_p(B_gathered.data_ptr()), int(shard_rows), int(shard_ld), int(shard_stride), int(n_cols),
                                              C.c_void_p(C_out.data_ptr()), int(ldc), c_layout, int(bool(accumulate)), C.c_void_p(st),
                                              int(algo), C.byref(dt) if timed else None))
        return dt.value if timed else None

    def prepare_b(self, B, n_cols, ldb=None, shard_rows=0, shard_stride=None, stream=None):
        """sparta_vbs_prepare_b: a B that stays the same over many products, prepared once (its row-major copy for the sparse-row kernels is
        made now instead of on every product).  Returns a PreparedB; B itself is referenced, not copied: keep it alive and unchanged."""
        import torch
        want_b = {_lib.F32: torch.float32, _lib.F16: torch.float16, _lib.BF16: torch.bfloat16}[self.dtype]
        if not (B.is_cuda and B.dtype == want_b and B.device.index == self.device and B.is_contiguous()):
            raise ValueError("B must be a contiguous %s tensor on device %d" % (want_b, self.device))
        if shard_rows:
            ldb = shard_rows if ldb is None else int(ldb)                      # gathered B: ldb = shard_ld, the column stride inside a slab (padded slabs: > shard_rows)
            shard_stride = ldb * n_cols if shard_stride is None else int(shard_stride)
            need = (self.cols // shard_rows - 1) * shard_stride + ldb * (n_cols - 1) + shard_rows
        else:
            ldb = self.cols if ldb is None else int(ldb)
            shard_stride, need = 0, ldb * n_cols
        if B.numel() < need:
            raise ValueError("B too small for the stated layout")
        st = torch.cuda.current_stream(self.device).cuda_stream if stream is None else stream
        h = C.c_void_p(None)
        check(lib.sparta_vbs_prepare_b(self.h, C.c_void_p(B.data_ptr()), int(ldb), int(shard_rows), int(shard_stride), int(n_cols), C.c_void_p(st), C.byref(h)))
        return PreparedB(self, h, B, int(n_cols))

    def spmm_prepared(self, Bp, C_out, accumulate=False, c_layout=_lib.COL_MAJOR, ldc=None, timed=False, stream=None):
        """sparta_vbs_spmm_prepared: C (+)= A * B for a PreparedB of this handle"""
        import torch
        if Bp.owner is not self or not Bp.h:
            raise ValueError("this B was prepared for another handle (or already closed)")
        if not (C_out.is_cuda and C_out.dtype == torch.float32 and C_out.device.index == self.device and C_out.is_contiguous()):
            raise ValueError("C must be a contiguous float32 tensor on device %d" % self.device)
        ldc = (self.rows if c_layout == _lib.COL_MAJOR else Bp.n_cols) if ldc is None else ldc
        if C_out.numel() < ldc * (Bp.n_cols if c_layout == _lib.COL_MAJOR else self.rows):
            raise ValueError("C too small")
        st = torch.cuda.current_stream(self.device).cuda_stream if stream is None else stream
        dt = C.c_float(0)
        check(lib.sparta_vbs_spmm_prepared(self.h, Bp.h, C.c_void_p(C_out.data_ptr()), int(ldc), c_layout, int(bool(accumulate)), C.c_void_p(st),
                                           C.byref(dt) if timed else None))
        return dt.value if timed else None

    def set_class_timing(self, enable=True):
        check(lib.sparta_vbs_set_class_timing(self.h, int(bool(enable))))

    def class_times(self):
        """ms of the last spmm per kernel (needs set_class_timing(True)).  Stream path (info()['last_path'] == 1):
        {'stream': main persistent kernel, 'fixup': split-tile fix-up}; generic path: per tile class {16, 32, 64}; 'sparse':
        the sparse-row kernels (+ the transposes of B / C they need), 0 when the handle has no such rows."""
        a = np.zeros(4, np.float32)
        check(lib.sparta_vbs_class_times(self.h, a.ctypes.data_as(_f32p)))
        if self.info()["last_path"] == 1:
            return {"stream": float(a[0]), "fixup": float(a[1]), "union": float(a[2]), "sparse": float(a[3])}      # 'union': the column-compacted tiles (k_union.hip; + the transpose of B when they ask for it first)
        if self.union_info()["area"] > 0 and self.info()["tiles64"] == 0:                     # (slot 2 is the column-compacted tiles' when no 64-row class ran)
            return {"class16": float(a[0]), "class32": float(a[1]), "union": float(a[2]), "sparse": float(a[3])}
        return {"class16": float(a[0]), "class32": float(a[1]), "class64": float(a[2]), "sparse": float(a[3])}

    def clock_mhz(self):
        """Shader clock (MHz) the product kernels of the last timed spmm ran at, keyed like class_times()
        (needs set_class_timing(True); 0.0 where no probe ran, e.g. the fix-up kernel)."""
        a = np.zeros(4, np.float64)
        check(lib.sparta_vbs_clock_mhz(self.h, a.ctypes.data_as(C.POINTER(C.c_double))))
        if self.info()["last_path"] == 1:
            return {"stream": float(a[0])}
        return {"class16": float(a[0]), "class32": float(a[1]), "class64": float(a[2])}

    def close(self):
        self._values_replaced()
        if self.h:
            lib.sparta_vbs_destroy(self.h)
            self.h = C.c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PreparedB:
    """sparta_b_t: a constant dense operand prepared for one handle (DeviceVBS.prepare_b)"""

    def __init__(self, owner, h, B, n_cols):
        self.owner, self.h, self.B, self.n_cols = owner, h, B, n_cols          # (keeps B alive)

    def close(self):
        if self.h:
            lib.sparta_b_destroy(self.h)
            self.h = C.c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _dense_layout(D):
    """(layout, ldd, dtype code) of a 2-D device tensor as the dense entries take it: one stride must be 1, the other at least the extent it steps over"""
    import torch
    codes = {torch.float32: _lib.F32, torch.float16: _lib.F16, torch.bfloat16: _lib.BF16}
    if not (hasattr(D, "is_cuda") and D.is_cuda and D.dim() == 2 and D.dtype in codes):
        raise ValueError("D must be a 2-D float32, float16 or bfloat16 tensor on the GPU")
    (rows, cols), (s0, s1) = D.shape, D.stride()
    if (s1 == 1 or cols <= 1) and (s0 >= cols or rows <= 1):
        return _lib.ROW_MAJOR, max(int(s0) if rows > 1 else 0, cols, 1), codes[D.dtype]
    if (s0 == 1 or rows <= 1) and (s1 >= rows or cols <= 1):
        return _lib.COL_MAJOR, max(int(s1) if cols > 1 else 0, rows, 1), codes[D.dtype]
    raise ValueError("D must have a stride of 1 along its rows or its columns and must not overlap itself (strides %r for shape %r): make it contiguous "
                     "yourself, nothing is copied silently" % (tuple(D.stride()), tuple(D.shape)))


def dense_block_ssq(D, row_part, block_col_size, out=None, timed=False, stream=None):
    """sparta_dense_block_ssq: the block scores of a dense matrix on the device, without a handle.  D: a 2-D float32, float16 or bfloat16 device tensor with
    one stride 1 (as DeviceVBS.gather_dense takes it); row_part: the first rows of the block-rows and, last, rows (block_rows + 1 non-decreasing entries
    from 0) as a sequence, a numpy array or a torch tensor (an int64 tensor on D's device is used as it is); block_col_size: w.  Returns a float64 tensor
    (block_rows, block_cols): per grid block the sum of the squares of its elements inside the matrix, what DeviceVBS.block_ssq gives for a stored block
    holding the same values.  One launch on torch's current stream, capturable.  Returns the scores, or (scores, kernel ms) if timed."""
    import torch
    layout, ldd, dt_code = _dense_layout(D)
    rows, cols = D.shape
    w = int(block_col_size)
    if w <= 0:
        raise ValueError("block_col_size must be > 0")
    if isinstance(row_part, torch.Tensor):
        rp = row_part.to(device=D.device, dtype=torch.int64).contiguous()
    else:
        rp = torch.as_tensor(np.ascontiguousarray(row_part, np.int64), device=D.device)
    if rp.dim() != 1 or rp.numel() < 1:
        raise ValueError("row_part must hold block_rows + 1 entries")
    block_rows, block_cols = rp.numel() - 1, ((cols - 1) // w + 1 if cols > 0 else 0)
    if out is None:
        out = torch.empty((block_rows, block_cols), dtype=torch.float64, device=D.device)
    elif not (out.is_cuda and out.dtype == torch.float64 and out.device == D.device and out.is_contiguous() and out.numel() == block_rows * block_cols):
        raise ValueError("out must be a contiguous float64 tensor of block_rows * block_cols = %d elements on D's device" % (block_rows * block_cols))
    with torch.cuda.device(D.device):
        st = torch.cuda.current_stream(D.device).cuda_stream if stream is None else stream
        dt = C.c_float(0)
        check(lib.sparta_dense_block_ssq(C.c_void_p(D.data_ptr() if D.numel() else None), ldd, layout, dt_code, int(rows), int(cols), block_rows, w,
                                         C.c_void_p(rp.data_ptr()), C.c_void_p(out.data_ptr() if out.numel() else None), C.c_void_p(st),
                                         C.byref(dt) if timed else None))
    out = out.view(block_rows, block_cols)
    return (out, dt.value) if timed else out


def sparsify(D, block_col_size, row_part=None, row_block_size=None, sparsity=None, mask=None, normalize=True, dtype=_lib.F32, device=None, updatable=True,
             transposable=True):
    """A dense layer made block-sparse on the device: -> (vbmat, handle, values).

    D: the dense weight matrix, a 2-D float32 / float16 / bfloat16 device tensor with one stride 1 (nn.Linear.weight as it is).  The grid: block columns of
    block_col_size, block-rows from row_part (block_rows + 1 entries from 0 to rows) or of row_block_size rows each (the last one shorter); one of the two.
    Which blocks are stored: those of `mask` ((block_rows, block_cols), non-zero = stored; a tensor or an array -- a pattern from elsewhere, a random SET
    pattern), or, with `sparsity`, the blocks prune.select keeps at that sparsity on the scores dense_block_ssq(D) -- divided by the block's elements inside
    the matrix when normalize, a block without an element scoring +Inf, as BlockPruner.scores does; the lowest scores go first, ties to the lower index.
    The mask is downloaded (one byte per grid block: the only host read), VBR.from_block_mask builds the pattern, to_device the handle (dtype, device --
    default D's --, updatable, transposable), gather_dense the values, set_values gives them to the handle.
    Returns the pattern-only VBR (its mab is zeros: the values live in `values`), the handle, and `values`: a float32 leaf tensor of nztot elements,
    requires_grad set, ready for vbs_linear, VbsSGD and VbsAdamW."""
    import torch
    from . import prune
    from .host import VBR
    _dense_layout(D)
    rows, cols = (int(x) for x in D.shape)
    w = int(block_col_size)
    if (row_part is None) == (row_block_size is None):
        raise ValueError("give exactly one of row_part and row_block_size")
    if (mask is None) == (sparsity is None):
        raise ValueError("give exactly one of sparsity and mask")
    if row_part is None:
        hb = int(row_block_size)
        if hb <= 0:
            raise ValueError("row_block_size must be > 0")
        row_part = np.minimum(np.arange(0, rows + hb, hb, dtype=np.int64), rows)[:(rows + hb - 1) // hb + 1]
    elif isinstance(row_part, torch.Tensor):
        row_part = row_part.detach().cpu().numpy()
    row_part = np.ascontiguousarray(row_part, np.int64).reshape(-1)
    block_rows, block_cols = len(row_part) - 1, (cols - 1) // w + 1
    if mask is None:
        rp_dev = torch.as_tensor(row_part, device=D.device)
        s = dense_block_ssq(D.detach(), rp_dev, w)
        if normalize:
            hts = (rp_dev[1:] - rp_dev[:-1]).to(torch.float64)
            wid = torch.clamp(cols - torch.arange(block_cols, device=D.device, dtype=torch.int64) * w, max=w).to(torch.float64)
            n_in = hts[:, None] * wid[None, :]
            s = torch.where(n_in > 0, s / n_in, torch.full_like(s, float("inf")))
        keep = prune.select([s.reshape(-1)], [torch.ones(s.numel(), dtype=torch.uint8, device=D.device)], float(sparsity), "layer")[0]
        mask = keep.reshape(block_rows, block_cols).cpu().numpy()                  # (synchronises: the one host read)
    elif isinstance(mask, torch.Tensor):
        mask = (mask.detach() != 0).to(torch.uint8).cpu().numpy()
    vbmat = VBR.from_block_mask(rows, cols, row_part, w, mask)
    dev = D.device.index if device is None else int(device)
    if dev != D.device.index:
        raise ValueError("device must be D's device (%d)" % D.device.index)
    handle = vbmat.to_device(dev, dtype=dtype, updatable=updatable, transposable=transposable)
    try:
        values = handle.gather_dense(D.detach())
        if updatable:
            handle.set_values(values)
        elif values.numel():
            # a handle that takes no new values is created from them: the gathered values go through the host once and vbmat.mab holds them
            vbmat.set_values(values.cpu().numpy())
            handle.close()
            handle = vbmat.to_device(dev, dtype=dtype, updatable=False, transposable=transposable)
    except Exception:
        handle.close()
        raise
    values.requires_grad_(True)
    return vbmat, handle, values


def repattern(vbmat, handle, tensors, keep=None, add=None, block_row_range=None):
    """A trained layer moved onto a new block pattern: the old pattern minus the blocks with keep[b] == 0 plus the blocks of `add` (VBR.repattern states the
    rule).  vbmat: the VBR whose arrays `handle` was created from (its pattern is what counts; its mab is not read); block_row_range: the range the handle was
    created with, if any; tensors: float32 device tensors in the handle's mab layout -- the values FIRST, then whatever shares their layout (momentum,
    exp_avg, exp_avg_sq).  Returns (new_vbmat, new_handle, new_tensors, map):
      new_vbmat    the new pattern (pattern only: its mab is all zero -- the values live in new_tensors[0])
      new_handle   an ordinary fresh handle of the old one's dtype, device, range and creation flags: the planner deals its steps anew and its images hold
                   what is kept; created from zeros, then given new_tensors[0] by set_values.  The old handle must be updatable.
      new_tensors  one torch.empty tensor per entry of `tensors`, filled by ONE move_blocks call per four tensors: kept blocks bit for bit, added blocks +0.0
      map          int32 numpy: per new block of the range the old block number, or -1
    If the old handle multiplies with its fp8 weight image (set_forward_a8) the new one is switched on as well -- and must qualify for it: whether a handle
    has the ONE stream image that holds every element depends on the pattern (an emptied block-row leaves its partner of a pair tile behind, a pattern of no
    block has no image at all).  Where the new pattern does not qualify the call raises SpartaError (unsupported) naming that reason, with the new handle
    closed and nothing else touched: switch the image off (set_forward_a8(False)) or choose another pattern.  The live set and the live switches are NOT
    carried: the new handle has no dead blocks unless the caller keeps some (BlockPruner.grow re-applies its own).  The old handle is left open and unchanged.
    This call synchronises: a keep given as a device tensor is downloaded, and move_blocks synchronises the stream.
    The two halves are repattern_prepare (everything that can refuse) and repattern_commit (the move): BlockPruner.compact prepares all its pairs first."""
    plan = repattern_prepare(vbmat, handle, tensors, keep=keep, add=add, block_row_range=block_row_range)
    return repattern_commit(plan)


class RepatternPlan:
    """what repattern_prepare hands to repattern_commit: the new pattern, the open new handle, the block map and the old side.  close() gives the new handle
    up (a plan that is not committed must be closed)"""

    def __init__(self, vbmat, handle, tensors, new_vbmat, new_handle, bmap, a8):
        self.vbmat, self.handle, self.tensors = vbmat, handle, list(tensors)
        self.new_vbmat, self.new_handle, self.bmap, self.a8 = new_vbmat, new_handle, bmap, a8

    def close(self):
        if self.new_handle is not None:
            self.new_handle.close()
            self.new_handle = None


def repattern_prepare(vbmat, handle, tensors, keep=None, add=None, block_row_range=None):
    """The first half of repattern, with its arguments: the checks, the host rule, the new handle, and -- if the old handle multiplies with its fp8 weight
    image -- whether the new one has the form for it (a8_info()["capable"]).  Moves nothing and changes nothing on the old side.  A refusal closes the new
    handle before it raises.  Returns a RepatternPlan for repattern_commit (or plan.close())."""
    if not handle.updatable:
        raise ValueError("repattern needs a handle created with updatable=True (the new handle takes the moved values through set_values)")
    if not tensors:
        raise ValueError("repattern needs at least the values tensor")
    if keep is not None and hasattr(keep, "detach"):
        keep = keep.detach().cpu().numpy()                     # (synchronises)
    new_vbmat, bmap = vbmat.repattern(keep=keep, add=add, block_row_range=block_row_range, values=False)
    a8 = bool(handle.dtype != _lib.F32 and handle.a8_info()["switch"])
    new_handle = DeviceVBS(new_vbmat, device=handle.device, dtype=handle.dtype, block_row_range=block_row_range, updatable=True,
                           transposable=handle.transposable)
    try:
        for i, t in enumerate(tensors):
            handle._prune_operand("tensor %d" % i, t)         # (what move_blocks would refuse in the middle of the commit)
        if a8 and not new_handle.a8_info()["capable"]:
            raise _lib.SpartaError(_lib.ERR_UNSUPPORTED, "repattern: the old handle multiplies with its fp8 weight image (set_forward_a8) and the new pattern does "
                                   "not qualify for one: its %d blocks do not lie in one stream image that holds every stored element (an emptied block-row "
                                   "leaves its partner of a pair tile behind; a pattern without a block has no image).  Nothing was changed: switch the image "
                                   "off first, or keep / add blocks so that the pattern qualifies" % new_handle.n_blocks)
    except Exception:
        new_handle.close()
        raise
    return RepatternPlan(vbmat, handle, tensors, new_vbmat, new_handle, bmap, a8)


def repattern_commit(plan):
    """The second half of repattern: the tensors moved in one move_blocks call per four, the fp8 switch set where the old handle has it on, the new handle
    given its values.  Returns (new_vbmat, new_handle, new_tensors, map).  A failure closes the new handle; the old side is never written."""
    import torch
    new_handle = plan.new_handle
    try:
        n = new_handle._nztot()
        new_tensors = [torch.empty(n, dtype=torch.float32, device=t.device) for t in plan.tensors]
        new_handle.move_blocks(plan.handle, plan.bmap, *zip(plan.tensors, new_tensors))
        if plan.a8:
            new_handle.set_forward_a8(True)
        new_handle.set_values(new_tensors[0])
    except Exception:
        plan.close()
        raise
    plan.new_handle = None
    return plan.new_vbmat, new_handle, new_tensors, plan.bmap


def vbs_multiply(vbmat, B, B_cols, C_out, n_streams=None, device=0):
    """Drop-in for the reference's GPU back-ends `f(const VBR&, DataT* B, int B_cols, DataT_C* C, float& dt[, n_streams])`
    (include/cuda_utilities.h:38-44): host B/C, C += A*B, returns dt in ms (kernel only). `n_streams` is accepted and
    ignored (there is one fused launch per tile class, not one GEMM per block)."""
    return vbmat.multiply(B, B_cols, C_out, device=device)
