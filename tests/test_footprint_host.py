"""tests/_footprint.py on the CPU: ALIGN_CASES is the covering list it claims to be and takes both sides of every alignment predicate of the product dispatch
at the shapes tests/test_footprint_gpu.py uses; check_untouched fails when a single word outside the defined elements changes, wherever it lies (a mutation
check of the checker); the integer operands keep every partial sum an integer below 2^24, so that "bit for bit" is the right bar.  No GPU."""
import itertools

import numpy as np
import pytest

import _footprint as F
import _util as U


# ---- ALIGN_CASES --------------------------------------------------------------------------------------------------------------------------------------
def test_align_cases_are_a_covering_list():
    cases = F.ALIGN_CASES
    assert 10 <= len(cases) <= 14 and len(set(cases)) == len(cases)
    assert {c[0] for c in cases} == {0, 4, 16, 76} and {c[2] for c in cases} == {0, 4, 8, 12}
    assert {c[1] for c in cases} == set(F.LDC_CLASSES) and {c[3] for c in cases} == set(F.LDB_CLASSES)
    assert {c[:2] for c in cases} == set(itertools.product(F.C_RESIDUES, F.LDC_CLASSES))
    assert {c[2:] for c in cases} == set(itertools.product(F.B_RESIDUES, F.LDB_CLASSES))


@pytest.mark.parametrize("used", [1, 5, 63, 128, 245, 251, 256, 425, 492, 512])
def test_leading_dimension_classes(used):
    r32, p4, odd = (F.ldc_of(used, c) for c in F.LDC_CLASSES)
    assert r32 % 32 == 0 and 0 <= r32 - used < 32 and p4 == r32 + 4 and odd % 2 == 1 and used < odd <= used + 2
    m4, od = F.ldb_of(used, "m4"), F.ldb_of(used, "odd")
    assert m4 % 4 == 0 and used < m4 <= used + 4 and od % 2 == 1 and used < od <= used + 2          # fp32: padding of at least one element, NaN in it
    m8, e2 = F.ldb_of(used, "m4", 2), F.ldb_of(used, "odd", 2)
    assert m8 % 8 == 0 and used < m8 <= used + 8 and e2 % 4 == 2 and used < e2 <= used + 4          # 16-bit: a multiple of 8; even but not a multiple of 4


def test_front_puts_the_operand_on_its_residue():
    for isz in (4, 2):
        for res in (0, 4, 8, 12, 16, 76):
            front = F.front_for(res, isz)
            assert F.MARGIN <= front < F.MARGIN + 128 // isz and (front * isz) % 128 == res
            a = F.arena(100, np.float32 if isz == 4 else np.float16, front, F.MARGIN, F.CANARY if isz == 4 else 0x7e00)
            assert len(a) == front + 100 + F.MARGIN and a.dtype.itemsize == isz
    with pytest.raises(AssertionError):
        F.arena(10, np.float32, 100, F.MARGIN, F.CANARY)          # an operand is never tightly bounded


def sides(shapes):
    """name -> the set of values the predicate takes over ALIGN_CASES at the given (rows of C, rows of B, n, C row-major, B row-major, element size of B)"""
    seen = {}
    for rows, cols, n, crm, brm, esz in shapes:
        for cr, cc, br, bc in F.ALIGN_CASES:
            ldc = F.ldc_of(n if crm else rows, cc)
            ldb = F.ldb_of(n if brm else cols, bc, esz)
            C = F.front_for(cr, 4) * 4                     # byte address of the operand in an arena that starts on a multiple of 256
            B = F.front_for(br, esz) * esz
            assert C % 128 == cr and B % 128 == br
            for k, val in F.predicates(C, ldc, B, ldb, n, crm, brm, esz).items():
                seen.setdefault(k, set()).add(bool(val))
    return seen


def test_every_host_predicate_takes_both_values():
    """at the shapes of tests/test_footprint_gpu.py: P32 251 x 245 and P64 425 x 492 at n = 128 (stream, ring, direct: the non-temporal stores), the smallest
    resident-column matrix 63 x 5 and PCSR 512 x 512 (vec_out, vec_in), the sparse rows at n = 256 with a row-major C (aligned(4), aligned(2)), a row-major fp32
    B (ensure_brm; the sparse rows' test of B itself)"""
    P32, P64, PCSR = F.int_geometry("P32"), F.int_geometry("P64"), F.int_csr("PCSR")[0]
    assert (P32.rows, P32.cols, P64.rows, P64.cols, PCSR.rows, PCSR.cols) == (251, 245, 425, 492, 512, 512)
    for rows, cols in ((251, 245), (425, 492)):
        s = sides([(rows, cols, 128, False, False, 4), (rows, cols, 128, False, False, 2)])
        assert s["c_nt"] == {True, False}, s
    for rows, cols, n in ((63, 5, 8), (512, 512, 8)):
        s = sides([(rows, cols, n, False, False, 4)])
        assert s["colres_vec_out"] == {True, False} and s["colres_vec_in"] == {True, False}, s
    for esz in (4, 2):
        s = sides([(512, 512, 256, True, False, esz)])                    # column-major B: the kernels read the library's own aligned copy
        assert s["sparse_aligned4"] == {True, False} and s["sparse_aligned2"] == {True, False}, s
    s = sides([(512, 512, 256, False, True, 4)])                          # row-major fp32 B read where it is, column-major C
    assert s["sparse_aligned4"] == {True, False} and s["sparse_aligned2"] == {True, False} and s["brm_in_place"] == {True, False}, s
    s = sides([(512, 512, 128, False, False, 4)])                         # n = 128 is no multiple of 256: never four elements per lane
    assert s["sparse_aligned4"] == {False} and s["sparse_aligned2"] == {True}, s
    s = sides([(432, 1024, 128, False, True, 4)])                         # PUNI with a row-major B: the column-compacted tiles read it in place or take a copy
    assert s["brm_in_place"] == {True, False}, s


# ---- check_untouched: the mutation check of the checker -----------------------------------------------------------------------------------------------
LINES, USED, LD = 7, 251, 256


def an_arena(front=None):
    front = F.front_for(76, 4) if front is None else front
    a = F.arena(LINES * LD, np.float32, front, F.MARGIN, F.CANARY)
    mask = F.place(a, front, np.full((LINES, USED), F.INTERIOR, np.uint32), LD)
    return a, mask, front


def test_check_untouched_passes_when_only_defined_elements_change():
    a, mask, front = an_arena()
    after = a.copy()
    after[mask] = F.bits_of(np.arange(mask.sum(), dtype=np.float32))
    assert mask.sum() == LINES * USED and mask[front] and not mask[front - 1] and not mask[front + USED] and mask[front + LD]
    F.check_untouched(after, a, mask)
    F.check_untouched(after.view(np.float32), a.view(np.float32), mask)          # (a float view: compared as uint32, NaN == NaN by its bits)


MUTATIONS = {       # name -> (offset from the first element of the operand, the region the message must name)
    "the last word of the front margin": (-1, "front margin"),
    "a word deep in the front margin": (-F.MARGIN + 3, "front margin"),
    "the ld padding of a middle line": (3 * LD + USED + 2, "ld padding"),
    "the element just behind the last column of the first line": (USED, "ld padding"),
    "the element just behind the last column of the last line": ((LINES - 1) * LD + USED, "ld padding"),
    "the first word of the back margin": (LINES * LD, "back margin"),
    "the last word of the arena": (LINES * LD + F.MARGIN - 1, "back margin"),
}


@pytest.mark.parametrize("name", sorted(MUTATIONS))
@pytest.mark.parametrize("flip", [1, 0x80000000, 0x00400000], ids=["low-bit", "sign-bit", "payload-bit"])
def test_check_untouched_fails_on_one_changed_word(name, flip):
    off, region = MUTATIONS[name]
    a, mask, front = an_arena()
    after = a.copy()
    after[mask] = F.bits_of(np.ones(mask.sum(), np.float32))
    after[front + off] ^= np.uint32(flip)                        # still a NaN: only a comparison of the bits sees it
    assert np.isnan(after.view(np.float32)[front + off]) and not mask[front + off]
    with pytest.raises(AssertionError) as e:
        F.check_untouched(after, a, mask, what=name)
    msg = str(e.value)
    assert "1 words outside the defined elements changed" in msg and "1 in the %s" % region in msg, msg
    assert "first (line, position): [(%d, %d)]" % divmod(off, LD) in msg, msg


def test_check_untouched_counts_and_names_every_region():
    a, mask, front = an_arena()
    after = a.copy()
    for off in (-5, -4, USED, LD + USED + 1, 2 * LD + LD - 1, LINES * LD + 7):
        after[front + off] = 0
    with pytest.raises(AssertionError) as e:
        F.check_untouched(after, a, mask)
    msg = str(e.value)
    assert "6 words" in msg and "2 in the front margin" in msg and "3 in the ld padding" in msg and "1 in the back margin" in msg, msg


def test_check_untouched_with_a_one_dimensional_interior():
    """G of sddmm and mab of set_values: one line, canaries on both sides"""
    front = F.front_for(4, 4)
    a = F.arena(1000, np.float32, front, F.MARGIN, F.CANARY)
    mask = F.interior_mask(len(a), front, 1, 1000, 1000)
    for off, region in ((-1, "front margin"), (1000, "back margin")):
        after = a.copy()
        after[front + off] ^= np.uint32(1)
        with pytest.raises(AssertionError) as e:
            F.check_untouched(after, a, mask)
        assert region in str(e.value)


# ---- the operands are integers whose partial sums stay below 2^24 -----------------------------------------------------------------------------------------
def test_integer_operands_make_every_order_of_additions_exact():
    """values and operands are integers of magnitude <= 3, C0 of magnitude <= 15: every partial sum of any subset of a product's terms, in any order, with or
    without C0, is an integer of magnitude <= 9 * (terms) + 15 < 2^24 and therefore exact in fp32 (the argument of tests/test_edge_geometry_host.py at these
    shapes); every operand is exact in f16 and bf16"""
    for key in ("P32", "P64", "P13", "P32G", "P64G"):
        v = F.int_geometry(key)
        assert np.array_equal(v.mab, np.round(v.mab)) and np.abs(v.mab).max() == 3 and (v.mab != 0).all()
        D = U.edge_dense(v)
        assert 3 * np.abs(D).sum(axis=1).max() + 15 < 2 ** 24 and 3 * np.abs(D).sum(axis=0).max() + 15 < 2 ** 24          # forward; spmm_t
        for dt in (1, 2):
            assert np.array_equal(U.edge_dense(v, dt), D)
    assert 9 * 128 + 15 < 2 ** 24                                                                                      # sddmm at k <= 128
    for which in ("PCSR", "PSPLIT", "PUNI"):
        m, g, w = F.int_csr(which)
        assert np.array_equal(m.vals, np.round(m.vals)) and np.abs(m.vals).max() == 3 and np.abs(m.vals).min() == 1
        assert 9 * int(np.diff(m.rowptr).max()) + 15 < 2 ** 24
    for shape, seed in (((245, 128), 1), ((425, 40), 2)):
        B, C0 = F.int_operand(shape, seed), F.int_c0(shape, seed)
        assert np.abs(B).max() == 3 and np.abs(C0).max() == 15 and np.array_equal(B, np.round(B))
        for bf16 in (False, True):
            back = F.bits_of(B, 2, bf16)
            f = back.view(np.float16).astype(np.float64) if not bf16 else (back.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
            assert np.array_equal(f, B)
    with pytest.raises(AssertionError):
        F.bits_of(np.array([1.0 + 2.0 ** -12]), 2, bf16=True)
