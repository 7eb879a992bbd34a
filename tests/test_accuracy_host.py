"""The accuracy bound of tests/_util.py: gamma_bound() holds for a plain fp32 evaluation in any order and is missed by arithmetics weaker than fp32, on every
input set that tests/test_accuracy_gpu.py hands the kernels (U.ACC_SETS).  No GPU involved.

Reference: numpy float64 L @ R (+ C0) on operands that are exactly representable in the storage type.  Products of two fp32 values have 48 significant bits and
the exponents span at most 2^-24 .. 2^26 (kind "wide"), so a float64 sum of up to ~1100 of them is exact to well below 2^-24 of sum|a||b|.

The three weaker arithmetics are required to MISS the bound on at least one checked element of every input set on which they differ from fp32 at all: the bf16
split and the 10-bit truncation are exact on operands that already fit their mantissa (bf16 data for both, fp16 data for the truncation), and are asserted to be
exact there instead.  Partial sums kept in fp16 miss it everywhere."""
import numpy as np
import pytest

import _util as U

IDS = [U.acc_id(s) for s in U.ACC_SETS]
MANT = {0: 24, 1: 11, 2: 8}                          # significant bits of the storage types


_plain = {}


def plain(s):
    """the ascending fp32 evaluation of the set (sum, smallest and largest magnitude met), computed once"""
    if s not in _plain:
        a = U.accuracy_set(s)
        _plain[s] = U.fp32_eval(a["L"], a["R"], track=True)
    return _plain[s]


def reference(a, with_c0):
    ref = a["L"] @ a["R"]
    return ref + a["C0"] if with_c0 else ref


def worst(got, ref, tol, check):
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(tol > 0, np.abs(got - ref) / np.where(tol > 0, tol, 1.0), np.where(got == ref, 0.0, np.inf))
    r = np.where(np.isfinite(got), r, np.inf)
    return float(r[check].max())


@pytest.mark.parametrize("s", U.ACC_SETS, ids=IDS)
def test_fp32_in_any_order_stays_inside_the_bound(s):
    a = U.accuracy_set(s)
    rng = np.random.default_rng(5)
    for name, order, with_c0 in (("ascending", None, False), ("descending", lambda ks: ks[::-1], True), ("random", lambda ks: rng.permutation(ks), False)):
        C0 = a["C0"] if with_c0 else None
        tol = U.gamma_bound(a["L"], a["R"], C0)
        got, lo, hi = plain(s) if name == "ascending" else U.fp32_eval(a["L"], a["R"], C0, order)
        assert worst(got, reference(a, with_c0), tol, a["check"]) <= 1.0, (name, worst(got, reference(a, with_c0), tol, a["check"]))
        # no product or partial sum leaves fp32's normal range (a condition on the inputs)
        assert name != "ascending" or (lo >= 2.0 ** -126 and hi < 2.0 ** 127), (name, lo, hi)          # (the products are the same in every order; the partial sums are tracked in one)
    # the bound is never looser than the suite's
    assert (tol <= 1e-5 * (np.abs(a["L"]) @ np.abs(a["R"]) + np.abs(a["C0"])) * (1 + 1e-12)).all()


@pytest.mark.parametrize("s", U.ACC_SETS, ids=IDS)
def test_inputs_exercise_short_sums(s):
    a = U.accuracy_set(s)
    K = U.gamma_terms(a["L"], a["R"])
    K = K[a["check"]]
    assert (K <= 4).mean() >= 0.25 and (K == 1).mean() >= 0.01, ((K <= 4).mean(), (K == 1).mean())
    dtype = s[2]
    for M in (a["L"], a["R"]):                       # every operand is what the storage type holds, in its normal range
        nz = np.abs(M[M != 0])
        assert np.array_equal(U.edge_round(M, dtype), M) and nz.min() >= (2.0 ** -14 if dtype == 1 else 2.0 ** -126) and nz.max() <= 65504.0


@pytest.mark.parametrize("weak", ["bf16-split", "trunc10", "fp16-sums"])
@pytest.mark.parametrize("s", U.ACC_SETS, ids=IDS)
def test_weaker_arithmetic_misses_the_bound(s, weak):
    a = U.accuracy_set(s)
    tol = U.gamma_bound(a["L"], a["R"])
    ref = reference(a, False)
    if weak == "fp16-sums":
        got, _, _ = U.fp32_eval(a["L"], a["R"], store=np.float16)
        exact_here = False
    else:
        got, _, _ = U.fp32_eval(a["L"], a["R"], product=U.weak_bf16_split if weak == "bf16-split" else U.weak_trunc10)
        exact_here = MANT[s[2]] <= (8 if weak == "bf16-split" else 11)
    if exact_here:                                   # the operands fit the mantissa this arithmetic keeps: it IS fp32 on them, and indistinguishable
        assert np.array_equal(got, plain(s)[0])
    else:
        assert worst(got, ref, tol, a["check"]) > 1.0, worst(got, ref, tol, a["check"])


def test_weaker_arithmetic_misses_the_bound_on_a_single_product():
    """the split's error is ~2^-16 per product, random in sign: 1e-5 * |a b| cannot see it, the bound at K = 1 (2^-23) does"""
    rng = np.random.default_rng(11)
    a, b = U.accuracy_draw(rng, 512, "wide", 0), U.accuracy_draw(rng, 512, "wide", 0)
    tol, K = U.gamma_bound(np.diag(a), np.diag(b)), U.gamma_terms(np.diag(a), np.diag(b))
    assert (np.diag(K) == 1).all()
    err = np.abs(U.weak_bf16_split(a, b).astype(np.float32).astype(np.float64) - a * b)
    assert (err <= 1e-5 * np.abs(a * b)).mean() > 0.5 and (err > np.diag(tol)).mean() > 0.9


# ---- edge_round against independent conversions, on the special values (to_h16 itself has no host entry point: tests/test_accuracy_gpu.py reads its image back) ------------------------------------------------------------------------------------
def same(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.where(np.isnan(a), 0.0, a), np.where(np.isnan(b), 0.0, b)) and np.array_equal(np.signbit(a) & ~np.isnan(a), np.signbit(b) & ~np.isnan(b))


def test_edge_round_on_the_special_values():
    torch = pytest.importorskip("torch")
    x = U.ACC_SPECIALS
    with np.errstate(over="ignore"):
        assert same(U.edge_round(x, 1), x.astype(np.float16).astype(np.float64))
    for dtype, tdt in ((1, torch.float16), (2, torch.bfloat16)):
        assert same(U.edge_round(x, dtype), torch.from_numpy(x.copy()).to(tdt).to(torch.float64).numpy()), dtype
    r16, rb = U.edge_round(x, 1), U.edge_round(x, 2)
    at = lambda v: int(np.flatnonzero(x == np.float32(v))[0])  # noqa: E731
    assert r16[at(65519.99)] == 65504.0 and np.isinf(r16[at(65520.0)]) and r16[at(1 + 2.0 ** -11)] == 1.0 and r16[at(1 + 3 * 2.0 ** -11)] == 1 + 2.0 ** -9
    assert r16[at(2.0 ** -25)] == 0.0 and r16[at(2.0 ** -24)] == 2.0 ** -24 and r16[at(1.5 * 2.0 ** -24)] == 2.0 ** -23 and r16[at(2.0 ** -14 - 2.0 ** -24)] == 2.0 ** -14 - 2.0 ** -24
    assert rb[at(1 + 2.0 ** -8)] == 1.0 and rb[at(1 + 3 * 2.0 ** -8)] == 1 + 2.0 ** -6 and rb[at(2.0 ** -134)] == 0.0 and rb[at(2.0 ** -133)] == 2.0 ** -133
    nan_in = np.isnan(x)
    assert nan_in.sum() == 8 and np.isnan(r16[nan_in]).all() and np.isnan(rb[nan_in]).all() and not np.isnan(r16[~nan_in]).any() and not np.isnan(rb[~nan_in]).any()
    assert np.isinf(rb[np.flatnonzero(x.view(np.uint32) == 0x7f7f8000)[0]]) and np.isfinite(rb[np.flatnonzero(x.view(np.uint32) == 0x7f7f7fff)[0]])
