"""Helpers of the footprint tests (tests/test_footprint_gpu.py, tests/test_footprint_host.py): arenas, alignment cases and the check that nothing outside the
defined elements of an output was written.  numpy only: no GPU, no torch.

An ARENA is one flat array of front + n_elems + back elements; the operand a product is given is the contiguous slice arena[front:front + n_elems], so it
starts in the middle of memory the test owns.  front and back are at least MARGIN elements: a stray access within 64 KiB (fp32) of either end of the operand
lands in the arena, where it is DETECTED -- a store changes a canary, a load brings a NaN into the result -- instead of faulting or vanishing into the
allocator's slack.  front holds up to 31 more elements (63 of a 16-bit operand) so that the operand starts at a chosen byte residue modulo 128 (the GPU test asserts that the arena
itself starts on a multiple of 256 bytes).

An operand is a matrix of `lines` lines of `used` elements, `ld` elements apart (columns of a column-major matrix, rows of a row-major one), n_elems = lines * ld.
Output arenas: the margins and the padding of ld hold CANARY (a quiet NaN with a payload, compared as uint32); the defined elements hold INTERIOR, another NaN
payload, before an overwriting call and a seeded integer C0 before an accumulating one.  Input arenas: margins, padding and the gap between the slabs of a
gathered B hold NaN, which a clean result must survive whatever a kernel loads there (0 * NaN is NaN)."""
import numpy as np

MARGIN = 16384
CANARY = 0x7fc5a5a5          # margins and ld padding of an output
INTERIOR = 0x7fc3c3c3        # the defined elements of an output before an overwriting call
DEAD = 0x7fc99999            # the elements of G in dead blocks before an accumulating sddmm with a live set: must keep these bits
QNAN = {"f32": 0x7fc00000, "f16": 0x7e00, "bf16": 0x7fc0}          # the NaN of an input arena, per type of the operand
UINT = {4: np.uint32, 2: np.uint16}


def front_for(residue_bytes, itemsize, margin=MARGIN):
    """the front margin (elements) that puts the operand at byte `residue_bytes` modulo 128 of an arena that starts on a multiple of 128"""
    assert 0 <= residue_bytes < 128 and residue_bytes % itemsize == 0 and (margin * itemsize) % 128 == 0
    return margin + residue_bytes // itemsize


def arena(n_elems, dtype, front, back, fill_bits):
    """one flat array of front + n_elems + back elements of the unsigned type as wide as dtype, every element fill_bits"""
    assert front >= MARGIN and back >= MARGIN, "an operand sits in the middle of its arena"
    return np.full(front + n_elems + back, fill_bits, UINT[np.dtype(dtype).itemsize])


def interior_mask(total, front, lines, used, ld):
    """bool over an arena of `total` elements: True on the defined elements of a lines x used matrix with leading dimension ld that starts at `front`"""
    assert used <= ld and front + lines * ld <= total
    m = np.zeros(total, bool)
    m[front:front + lines * ld].reshape(lines, ld)[:, :used] = True
    return m


def place(a, front, M, ld):
    """write the lines of M (lines x used, already in the arena's bit type) into arena a at `front` with leading dimension ld; returns the interior mask"""
    lines, used = M.shape
    a[front:front + lines * ld].reshape(lines, ld)[:, :used] = M
    return interior_mask(len(a), front, lines, used, ld)


def bits_of(M, itemsize=4, bf16=False):
    """float64 / float32 values (exact in the target type) as the bits of fp32 (itemsize 4), fp16 or bf16 (itemsize 2)"""
    f = np.ascontiguousarray(M, np.float32)
    if itemsize == 4:
        return f.view(np.uint32)
    if bf16:
        u = f.view(np.uint32)
        assert not (u & 0xffff).any(), "not exact in bf16"
        return (u >> 16).astype(np.uint16)
    h = f.astype(np.float16)
    assert np.array_equal(h.astype(np.float32), f), "not exact in fp16"
    return h.view(np.uint16)


def region_of(idx, front, n_elems, ld):
    """where element idx of an arena lies: 'front margin', 'ld padding' (anything inside the operand that is not a defined element) or 'back margin'"""
    return "front margin" if idx < front else "back margin" if idx >= front + n_elems else "ld padding"


def check_untouched(arena_after, arena_before, interior, front=None, ld=None, what=""):
    """every element outside `interior` has the bits it had before the call.  On failure: how many words changed, where they lie (front margin, ld padding,
    back margin) and the first few (line, position) pairs -- line and position inside the operand (negative / past the last line: in a margin)"""
    a = np.ascontiguousarray(arena_after).view(UINT[arena_after.dtype.itemsize])
    b = np.ascontiguousarray(arena_before).view(UINT[arena_before.dtype.itemsize])
    assert a.shape == b.shape == interior.shape
    bad = np.flatnonzero((a != b) & ~interior)
    if len(bad) == 0:
        return
    inside = np.flatnonzero(interior)
    front = int(inside[0]) if front is None and len(inside) else (0 if front is None else front)
    n_elems = (int(inside[-1]) + 1 - front) if len(inside) else 0
    if ld is None:          # the distance between the first elements of the first two lines
        starts = inside[np.concatenate([[True], np.diff(inside) > 1])] if len(inside) else inside
        ld = int(starts[1] - starts[0]) if len(starts) > 1 else max(n_elems, 1)
    n_elems = -(-n_elems // ld) * ld if n_elems else 0
    where = {}
    for i in bad:
        r = region_of(int(i), front, n_elems, ld)
        where[r] = where.get(r, 0) + 1
    first = [tuple(int(x) for x in divmod(int(i) - front, ld)) for i in bad[:6]]
    raise AssertionError("%s: %d words outside the defined elements changed: %s; first (line, position): %s; e.g. 0x%08x -> 0x%08x"
                         % (what, len(bad), ", ".join("%d in the %s" % (n, r) for r, n in sorted(where.items())), first, int(b[bad[0]]), int(a[bad[0]])))


# ---- alignment cases -----------------------------------------------------------------------------------------------------------------------------------
C_RESIDUES = (0, 4, 16, 76)                  # bytes modulo 128 at which the output starts
B_RESIDUES = (0, 4, 8, 12)                   # ... and the input (multiples of 4 bytes: a 16-bit operand on an odd element is refused, never run)
LDC_CLASSES = ("r32", "r32+4", "odd")        # the used length rounded up to a multiple of 32; that + 4; odd
LDB_CLASSES = ("m4", "odd")                  # fp32: a multiple of 4; odd.  16-bit operands: a multiple of 8; even but not a multiple of 4


def _cover():
    cs = [(r, c) for c in LDC_CLASSES for r in C_RESIDUES]                    # every pair (C residue, ldc class): 12
    bs = [(r, c) for r in B_RESIDUES for c in LDB_CLASSES]                    # every pair (B residue, ldb class): 8, dealt round-robin over the 12
    return tuple((cr, cc) + bs[(i + i // len(bs)) % len(bs)] for i, (cr, cc) in enumerate(cs))


ALIGN_CASES = _cover()                       # (c_residue_bytes, ldc_class, b_residue_bytes, ldb_class): a covering list, not the full cross


def ldc_of(used, cls):
    r32 = (used + 31) // 32 * 32
    return {"r32": r32, "r32+4": r32 + 4, "odd": used + 1 + (used & 1)}[cls]


def ldb_of(used, cls, itemsize=4):
    """fp32: m4 = the next multiple of 4 above used, odd = the next odd number above used.  16-bit: m4 stands for 'a multiple of 8', odd for 'even but not a
    multiple of 4' (an odd leading dimension is refused for 16-bit operands)"""
    if itemsize == 4:
        return {"m4": used // 4 * 4 + 4, "odd": used + 1 + (used & 1)}[cls]
    x = used // 4 * 4 + 2
    return {"m4": used // 8 * 8 + 8, "odd": x if x > used else x + 4}[cls]


# ---- the host predicates of the dispatch, as Python expressions (tests/test_footprint_host.py proves ALIGN_CASES takes both sides of each) ---------------
def predicates(C, ldc, B, ldb, n, c_row_major, b_row_major, esz=4):
    """C, B: byte addresses.  Copied from sparta_amd/csrc/vbs_capi.cpp; the comment names the function and the expression"""
    per16 = 16 // esz
    v_ok = lambda v: (n % (64 * v) == 0 and (not b_row_major or (ldb % v == 0 and B % (esz * v) == 0))          # noqa: E731
                      and (not c_row_major or (ldc % v == 0 and C % (4 * v) == 0)))
    return {
        # c_store_nt(): return !c_row_major && (...) && ldc % 32 == 0 && ((uintptr_t)C % 128) == 0;
        "c_nt": (not c_row_major) and ldc % 32 == 0 and C % 128 == 0,
        # launch_sparse_rows(), the resident-column launch: cp.vec_out = ldc % 4 == 0 && ((uintptr_t)dC % 16) == 0
        "colres_vec_out": ldc % 4 == 0 and C % 16 == 0,
        # launch_sparse_rows(), the resident-column launch: cp.vec_in = ldb % 4 == 0 && ((uintptr_t)dB % 16) == 0
        "colres_vec_in": ldb % 4 == 0 and B % 16 == 0,
        # launch_sparse_rows(): auto aligned = [&](int v) { out_ok = q.out_is_c == 2 || (q.ldo % v == 0 && out % (4 * v) == 0);
        #     return n_cols % (64 * v) == 0 && q.ldb % v == 0 && out_ok && q.B % (esz * v) == 0; }
        # (q.B, q.ldb: the caller's B when it is row-major, else the library's own 16-byte aligned copy; out_is_c == 2: a column-major C)
        "sparse_aligned4": v_ok(4),
        "sparse_aligned2": v_ok(2),
        # ensure_brm(): b_row_major && shard_rows == 0 && (!aligned16 || (ldb % per16 == 0 && ((uintptr_t)dB % 16) == 0)) -> B is read in place
        "brm_in_place": b_row_major and ldb % per16 == 0 and B % 16 == 0,
    }


# ---- the matrices: the poison geometries of tests/_util.py with the integer values of the edge geometries -------------------------------------------------
_geo = {}


def int_geometry(key):
    """poison geometry `key` (P32, P64, P13, P32G, P64G) with seeded values -3 .. 3 without a zero inside the stored blocks (U._edge_values 'int': the stored
    positions past cols are non-zero too), exact in f16 and bf16"""
    import _util as U
    if key not in _geo:
        v = U.poison_geometries()[key]
        arr = (v.rows, v.cols, int(v.block_col_size), v.row_part, v.nzcount, v.jab)
        _geo[key] = U.sa_vbr(arr, U._edge_values(arr, "int", 7400 + sorted(U.poison_geometries()).index(key)))
    return _geo[key]


def int_csr(which):
    """(CSR, grouping, w) of PCSR / PSPLIT / PUNI (tests/_util.py) with seeded values in {-3 .. 3} \\ {0}"""
    import _util as U
    import sparta_amd as sa
    if which not in _geo:
        m, g, w = {"PCSR": U.poison_csr, "PSPLIT": U.poison_split, "PUNI": U.poison_union}[which]()
        vals = np.random.default_rng(7450 + len(which)).integers(1, 4, m.nztot()).astype(np.float32)
        vals *= np.random.default_rng(7460).choice([-1.0, 1.0], m.nztot()).astype(np.float32)
        _geo[which] = (sa.CSR(m.rows, m.cols, np.asarray(m.rowptr, np.int64), np.asarray(m.colidx, np.int32), vals), g, w)
    return _geo[which]


def int_operand(shape, seed):
    """seeded integers -3 .. 3 as float64: exact in fp32, f16 and bf16"""
    return np.random.default_rng(seed).integers(-3, 4, shape).astype(np.float64)


def int_c0(shape, seed):
    """the previous content of an accumulating output: seeded integers -15 .. 15 (multiples of 5, as tests/test_edge_geometry_gpu.py)"""
    return int_operand(shape, seed) * 5.0
