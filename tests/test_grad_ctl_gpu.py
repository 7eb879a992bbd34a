"""Device-side gradient clipping and loss scaling on the GPU (k_gradctl.hip, and the control record inside the steps of k_update.hip).

sparta_grad_stats is held to the bound of ANY summation order of exact fp64 squares; sparta_grad_ctl_finish to grad_ctl_ref (tests/test_grad_ctl_host.py) bit for
bit; the steps under control to sgd_ref / adam_ref with g * coef inserted and coef read back from the record; a skipped step to "nothing moved, the handle
holds W"; the captured sequence [stats, finish, adam_step_ctl] to an eager run of the same calls through a replay whose gradient has become non-finite.  The
matrices, canary buffers and product helpers are those of tests/test_sgd_step_gpu.py / tests/test_adam_step_gpu.py and the files they draw on."""
import ctypes as C
import functools

import numpy as np
import pytest

import sparta_amd as sa
from sparta_amd import _lib
from sparta_amd._lib import lib
from sparta_amd.autograd import vbs_linear

torch = pytest.importorskip("torch")

from test_set_values_gpu import TDT, DT_ID, dense_b, product  # noqa: E402
from test_spmm_t_gpu import with_values, run_t, dense_x, hub_env  # noqa: E402
import test_sgd_step_gpu as tsgd  # noqa: E402
from test_sgd_step_gpu import CANARY, FUSED, build_all, sgd_ref, same_bits, make  # noqa: E402
import test_adam_step_gpu as tadam  # noqa: E402
from test_adam_step_gpu import draw_w, draw_g, assert_state  # noqa: E402
from test_adam_step_host import adam_ref, fresh_state  # noqa: E402
from test_grad_ctl_host import stats_ref, grad_ctl_ref, fresh_record, record_fields  # noqa: E402

pytestmark = pytest.mark.gpu

f32 = np.float32
_f32p = C.POINTER(C.c_float)
WORDS = _lib.GRAD_CTL_BYTES // 4
CHUNK, MAX_GRID = _lib.GRAD_STATS_CHUNK, _lib.GRAD_STATS_MAX_GRID
RPAD = 66                                                            # floats around R: 264 bytes, so R sits on an 8-byte boundary that is no 16-byte one
# The launch rule (include/sparta_amd.h, vbs_gradctl_stats_kernel): min(ceil(n / CHUNK), MAX_GRID) workgroups; behind a head of up to 3 elements the 16-byte
# loads go in WHOLE chunks of CHUNK elements, dealt round-robin (workgroup b takes chunks b, b + grid, ...), and a last partial chunk.  A workgroup makes a
# second trip through its loop over whole chunks, accumulators carried over, as soon as there are MAX_GRID + 1 whole chunks behind the head: the smallest
# such n is CHUNK * (MAX_GRID + 1) + head, and with the longest head, 3, every alignment has them.
SECOND_TRIP = CHUNK * (MAX_GRID + 1) + 3
assert SECOND_TRIP <= 5_000_000


def whole_chunks(n, pad):
    """whole chunks of 16-byte loads for n floats starting `pad` floats behind a 16-byte boundary, by the rule above"""
    head = min(n, (-pad) % 4)
    return (n - head) // CHUNK


@pytest.fixture(scope="module")
def mats():
    return build_all()


class Record:
    """R as a slice of a canary buffer; words(): the 16 words of the record (asserts the canaries)"""

    def __init__(self, words=None):
        self.buf = torch.full((WORDS + 2 * RPAD,), CANARY, dtype=torch.float32, device="cuda")
        self.R = self.buf[RPAD:RPAD + WORDS]
        assert self.R.data_ptr() % 16 == 8
        self.R.zero_()
        if words is not None:
            self.write(words)

    def write(self, words):
        self.R[:16].copy_(torch.from_numpy(np.asarray(words).view(f32).copy()))

    def ptr(self):
        return C.c_void_p(self.R.data_ptr())

    def words(self):
        torch.cuda.synchronize()
        h = self.buf.cpu().numpy()
        assert np.all(h[:RPAD] == CANARY) and np.all(h[-RPAD:] == CANARY), "a write outside R"
        return h[RPAD:RPAD + 16].view(np.uint32).copy()


class Grad:
    """n floats at `pad` floats into a canary buffer: pad = 66 an 8-byte boundary that is no 16-byte one, 67 a 4-byte one"""

    def __init__(self, G, pad):
        n = len(G)
        self.n, self.pad = n, pad
        self.buf = torch.full((n + 2 * pad,), CANARY, dtype=torch.float32, device="cuda")
        self.G = self.buf[pad:pad + n]
        if n:
            assert self.G.data_ptr() % 16 == (4 * pad) % 16 != 0
        self.G.copy_(torch.from_numpy(np.array(G, f32)))

    def check(self):
        h = self.buf.cpu().numpy()
        assert np.all(h[:self.pad] == CANARY) and np.all(h[self.pad + self.n:] == CANARY), "a write outside G"


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def grad_stats(G, rec, accumulate):
    """G: a device tensor, or None with n = 0"""
    n = 0 if G is None else G.numel()
    p = None if n == 0 else C.cast(C.c_void_p(G.data_ptr()), _f32p)
    sa._lib.check(lib.sparta_grad_stats(p, n, rec.ptr(), int(accumulate), stream(), None))


def finish(rec, cfg):
    c = _lib.GradCtlCfg(cfg.get("max_norm", 0.0), cfg.get("growth_factor", 2.0), cfg.get("backoff_factor", 0.5), cfg.get("growth_interval", 0))
    sa._lib.check(lib.sparta_grad_ctl_finish(rec.ptr(), C.byref(c), stream()))


@functools.lru_cache(maxsize=None)
def drawn(n, seed=0):
    """n values drawn like draw_g plus a few subnormals, and their stats_ref: computed once per size"""
    rng = np.random.default_rng(1000 + n % 9973 + seed)
    G = draw_g(rng, n)
    if n >= 3:
        at = rng.choice(n, min(n, 5), replace=False)
        G[at] = np.array([1e-40, -3e-42, 1.4e-45, 7e-39, -1e-38], f32)[:len(at)]
        assert np.all(np.abs(G[at]) < np.finfo(f32).tiny) and np.all(G[at] != 0)
    G.setflags(write=False)
    return G, stats_ref(G)


def within(ssq, want, n):
    """any order of summing n exact squares in fp64: n - 1 additions, each a relative 2^-53 on a partial sum of non-negative terms, none above the total"""
    return abs(ssq - want) <= n * 2.0 ** -53 * want


# ---- 1. stats ----------------------------------------------------------------------------------------------------------------------------------------
SIZES = [0, 1, 3, 4, 5, 255, 257, CHUNK - 1, CHUNK, CHUNK + 1, SECOND_TRIP]


@pytest.mark.parametrize("pad", [66, 67], ids=["align8", "align4"])
@pytest.mark.parametrize("n", SIZES)
def test_stats_sizes(n, pad):
    G, (want, _) = drawn(n)
    g = Grad(G, pad)
    if n == SECOND_TRIP:                                             # workgroup 0 takes chunk 0 and chunk MAX_GRID; one element fewer and nobody makes a second trip
        assert whole_chunks(n, pad) == MAX_GRID + 1 and whole_chunks(CHUNK * (MAX_GRID + 1) - 1, pad) == MAX_GRID
    junk = fresh_record(ssq=123.0, nonfinite=7)
    junk[3] = 99
    rec = Record(junk)
    grad_stats(g.G if n else None, rec, 0)
    w = rec.words()
    g.check()
    r = record_fields(w)
    print("n = %d: ssq %.17g, fsum %.17g, |diff| / fsum = %.3g (bound %.3g)" % (n, r["ssq"], want, abs(r["ssq"] - want) / want if want else 0.0, n * 2.0 ** -53))
    assert r["nonfinite"] == 0 and w[3] == 0
    assert within(r["ssq"], want, n), (n, r["ssq"], want)
    if n > 0:
        assert r["ssq"] > 0
    grad_stats(g.G if n else None, rec, 0)                            # a second run: the same bits
    assert np.array_equal(rec.words(), w)


def test_stats_counts_nonfinite_elements():
    """Inf / NaN / -Inf at the first, the last and the chunk-boundary positions (on both sides of each boundary, for every head the alignment can give)"""
    n = 3 * CHUNK + 5
    G0, _ = drawn(n)
    for pad in (66, 67):
        G = G0.copy()
        at = sorted({0, n - 1} | {c * CHUNK + d for c in (1, 2, 3) for d in (-1, 0, 1, 2, 3, 4) if c * CHUNK + d < n})
        G[at] = np.resize(np.array([np.inf, np.nan, -np.inf], f32), len(at))
        want, k = stats_ref(G)
        assert k == len(at) >= 14
        g = Grad(G, pad)
        rec = Record()
        grad_stats(g.G, rec, 0)
        r = record_fields(rec.words())
        assert r["nonfinite"] == k, (pad, r)
        assert np.isfinite(r["ssq"]) and within(r["ssq"], want, n), (pad, r["ssq"], want)


def test_stats_accumulate_is_the_concatenation():
    parts = [drawn(1000)[0].copy(), drawn(CHUNK + 1)[0].copy(), drawn(13, seed=1)[0].copy()]
    parts[0][17] = np.inf
    parts[2][[0, 12]] = np.nan
    want, k = stats_ref(np.concatenate(parts))
    assert k == 3
    rec = Record(fresh_record(ssq=55.0, nonfinite=9))
    gs = [Grad(p, 67) for p in parts]
    for i, g in enumerate(gs):
        grad_stats(g.G, rec, i > 0)
    r = record_fields(rec.words())
    assert r["nonfinite"] == 3 and within(r["ssq"], want, sum(len(p) for p in parts)), (r, want)
    w = rec.words()
    grad_stats(None, rec, 1)                                          # nothing to add
    assert np.array_equal(rec.words(), w)
    grad_stats(None, rec, 0)                                          # n = 0 starts over
    assert not rec.words()[:4].any()
    for g in gs:
        g.check()


def test_stats_timed_and_refusals():
    G, (want, _) = drawn(CHUNK + 1)
    g, rec = Grad(G, 67), Record()
    dt = C.c_float(-1.0)
    sa._lib.check(lib.sparta_grad_stats(C.cast(C.c_void_p(g.G.data_ptr()), _f32p), g.n, rec.ptr(), 0, stream(), C.byref(dt)))
    assert dt.value > 0.0 and within(record_fields(rec.words())["ssq"], want, g.n)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        gph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gph, stream=s):
            rc = lib.sparta_grad_stats(C.cast(C.c_void_p(g.G.data_ptr()), _f32p), g.n, rec.ptr(), 0, stream(), C.byref(dt))
            grad_stats(g.G, rec, 1)                                  # (the capture goes on: the refusal launched nothing)
        assert rc == _lib.ERR_UNSUPPORTED and "captured" in lib.sparta_last_error().decode()
        gph.replay()
    r = record_fields(rec.words())
    assert within(r["ssq"], 2 * want, 2 * g.n)


# ---- 2. finish ---------------------------------------------------------------------------------------------------------------------------------------
FINISH_CASES = {
    "clip_inactive": (fresh_record(1.0, 4.0), dict(max_norm=5.0)),
    "clip_active": (fresh_record(8.0, 1234.567), dict(max_norm=1.0)),
    "max_norm_0": (fresh_record(4.0, 1e30), dict(max_norm=0.0)),
    "nonfinite": (fresh_record(2.0, 9.0, nonfinite=3, skipped_total=5), dict(max_norm=1.0)),
    "root_overflows": (fresh_record(1.0, 1e80), dict(max_norm=1.0)),
    "norm_overflows_scale_below_1": (fresh_record(0.25, 9e76), dict(max_norm=1.0)),
    "growth_reaches_interval": (fresh_record(1024.0, 9.0, growth_tracker=1), dict(growth_interval=2, growth_factor=2.0)),
    "growth_not_yet": (fresh_record(1024.0, 9.0, growth_tracker=0), dict(growth_interval=2, growth_factor=1.5)),
    "growth_refused": (fresh_record(2.0 ** 127, 9.0, growth_tracker=1), dict(growth_interval=2)),
    "backoff": (fresh_record(1024.0, 9.0, nonfinite=1, growth_tracker=1), dict(growth_interval=2, backoff_factor=0.75)),
    "zero_scale_word": (fresh_record(None, 7.0), dict(max_norm=0.5, growth_interval=1, growth_factor=3.0)),
    "inexact_scale": (fresh_record(3.0, 0.37), dict(max_norm=0.1)),
}


@pytest.mark.parametrize("case", sorted(FINISH_CASES))
def test_finish_bit_exact(case):
    words, cfg = FINISH_CASES[case]
    words = words.copy()
    words[10:] = 0xdeadbeef                                          # finish writes them as zero
    rec = Record(words)
    finish(rec, cfg)
    got, want = rec.words(), grad_ctl_ref(words, cfg)
    assert np.array_equal(got, want), (case, record_fields(got), record_fields(want), got.tolist(), want.tolist())
    finish(rec, cfg)                                                 # and once more from the record it left
    assert np.array_equal(rec.words(), grad_ctl_ref(want, cfg)), case


# ---- 3. the steps under control ----------------------------------------------------------------------------------------------------------------------
# an fp32 handle whose fragment kernel owns the step, an fp32 handle with 33..64-row tiles (two-pass form), a 16-bit pair-tile handle, the hub handle
STEP_CASES = [("padded", sa.F32), ("jaccard", sa.F32), ("pairs", sa.F16), ("hub", sa.BF16)]
STEP_IDS = ["%s-%s" % (k, DT_ID[dt]) for k, dt in STEP_CASES]
# coef == inv (no clipping, an exact and an inexact 1 / s), and clipped
CTL_CONFIGS = [dict(loss_scale=4.0), dict(loss_scale=3.0), dict(loss_scale=1.0, max_norm=1.0), dict(loss_scale=8.0, max_norm=0.5)]


def set_fuse(monkeypatch, fuse):
    for var in ("SPARTA_SGD_FUSE", "SPARTA_ADAM_FUSE"):
        if fuse is None:
            monkeypatch.delenv(var, raising=False)
        else:
            monkeypatch.setenv(var, fuse)


def control(G_dev, G_host, ctl_cfg, rec=None):
    """stats + finish on the device; returns (rec, the 16 words).  The words are what grad_ctl_ref gives from the statistics the DEVICE computed (ssq may
    differ from fsum in its last bits, within the bound of test_stats_sizes)."""
    rec = rec or Record(fresh_record(ctl_cfg["loss_scale"]))
    grad_stats(G_dev, rec, 0)
    before = rec.words()
    want, k = stats_ref(G_host)
    r = record_fields(before)
    assert r["nonfinite"] == k and within(r["ssq"], want, len(G_host))
    finish(rec, ctl_cfg)
    after = rec.words()
    assert np.array_equal(after, grad_ctl_ref(before, ctl_cfg))
    return rec, after


def scaled(G, grad_scale, coef):
    """g = g * grad_scale (if != 1), then g = g * coef: one rounding each"""
    g = np.asarray(G, f32)
    if grad_scale != 1:
        g = g * f32(grad_scale)
    return g * f32(coef)


@pytest.mark.parametrize("fuse", [None, "1", "0"], ids=["default", "fuse1", "fuse0"])
@pytest.mark.parametrize("key,dtype", STEP_CASES, ids=STEP_IDS)
def test_steps_bit_exact_under_control(mats, key, dtype, fuse, monkeypatch):
    hub_env(monkeypatch, key)
    set_fuse(monkeypatch, fuse)
    v = mats[key]
    n = int(v.nztot)
    rng = np.random.default_rng(400)
    H = make(v, dtype)
    if key == "hub":
        assert H.hub_info()["steps"] > 0
    seen = set()
    # Adam: weight decay and a grad_scale of its own in front of coef
    cfg = dict(lr=1e-2, weight_decay=0.01, grad_scale=0.5)
    W = draw_w(v, 20)
    op = tadam.Operands(n, W, np.zeros(n, f32))
    ref = (W, np.zeros(n, f32), np.zeros(n, f32), fresh_state())
    for ci, ctl_cfg in enumerate(CTL_CONFIGS):
        G = draw_g(rng, n)
        op.set_grad(G)
        rec, words = control(op.G, G, ctl_cfg)
        r = record_fields(words)
        assert r["skip"] == 0 and (float(r["coef"]) == float(f32(1) / f32(ctl_cfg["loss_scale"]))) == ("max_norm" not in ctl_cfg), (ci, r)
        seen.add("clipped" if "max_norm" in ctl_cfg else "unclipped")
        H.adam_step(*op.args(), ctl=rec.R, **cfg)
        ref = adam_ref(ref[0], scaled(G, cfg["grad_scale"], r["coef"]), ref[1], ref[2], ref[3], dict(cfg, grad_scale=1.0))
        assert_state(op.read(), ref, (key, "adam", ci))
        assert np.array_equal(rec.words(), words)                    # the step reads R, it does not write it
        info = H.step_info()
        if fuse is not None:
            assert info["fused"] == (FUSED[(key, dtype)] if int(fuse) else 0), (key, info)
        assert info["launches"] == 2 if info["fused"] else info["launches"] >= 3, (key, info)
    assert seen == {"clipped", "unclipped"}
    # SGD with momentum
    cfg = dict(lr=0.25, momentum=0.9, weight_decay=0.01)
    W = draw_w(v, 21)
    sop = tsgd.Operands(n, W, np.zeros(n, f32))
    M = np.zeros(n, f32)
    for ci, ctl_cfg in enumerate(CTL_CONFIGS):
        G = draw_g(rng, n)
        sop.set_grad(G)
        rec, words = control(sop.G, G, ctl_cfg)
        H.sgd_step(sop.W, sop.G, sop.M, ctl=rec.R, **cfg)
        W, M = sgd_ref(W, scaled(G, 1.0, record_fields(words)["coef"]), M, **cfg)
        Wd, Md = sop.read()
        assert same_bits(Wd, W) and same_bits(Md, M), (key, "sgd", ci)
        info = H.step_info()
        assert info["launches"] == 1 if info["fused"] else info["launches"] >= 2, (key, info)
    H.close()


def test_step_refuses_a_misaligned_record(mats):
    v = mats["padded"]
    n = int(v.nztot)
    H = make(v, sa.F32)
    W0 = draw_w(v, 22)
    op = tadam.Operands(n, W0, draw_w(v, 23))
    rec = Record(fresh_record(1.0))
    f = [C.cast(C.c_void_p(t.data_ptr()), _f32p) for t in (op.W, op.G, op.M, op.V)]
    off4 = C.c_void_p(rec.R.data_ptr() + 4)
    rc = lib.sparta_vbs_adam_step_ctl(H.h, *f, C.c_void_p(op.S.data_ptr()), C.byref(_lib.AdamCfg(1e-2, 0.9, 0.999, 1e-8, 0.0, 1.0, 1, 0)), off4, None, None)
    assert rc == _lib.ERR_INVALID and "sparta_vbs_adam_step_ctl" in lib.sparta_last_error().decode() and "8-byte" in lib.sparta_last_error().decode()
    rc = lib.sparta_vbs_sgd_step_ctl(H.h, f[0], f[1], f[2], C.byref(_lib.SgdCfg(0.5, 0.9, 0.0, 1.0)), off4, None, None)
    assert rc == _lib.ERR_INVALID and "sparta_vbs_sgd_step_ctl" in lib.sparta_last_error().decode()
    assert H.step_info()["fused"] == -1                              # nothing ran
    got = op.read()
    assert same_bits(got[0], W0) and not got[1].any() and not got[2].any() and not got[3].any()
    with pytest.raises(ValueError):
        H.adam_step(*op.args(), lr=1e-2, ctl=torch.zeros(16, dtype=torch.int32, device="cuda"))      # not a whole record
    H.close()


# ---- 4. skip -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fuse", [None, "0"], ids=["default", "fuse0"])
@pytest.mark.parametrize("key,dtype", STEP_CASES, ids=STEP_IDS)
def test_skipped_step_moves_nothing_and_writes_the_handle_from_w(mats, key, dtype, fuse, monkeypatch):
    hub_env(monkeypatch, key)
    set_fuse(monkeypatch, fuse)
    monkeypatch.setenv("SPARTA_PATH", "stream")                      # one product path for both handles, as tests/test_adam_step_gpu.py::test_products_follow
    v = mats[key]
    n = int(v.nztot)
    rng = np.random.default_rng(500)
    B, X = dense_b(v, 128, 501, integer=False), dense_x(v.rows, 128, 502, integer=False)
    other = torch.from_numpy(draw_w(v, 31)).cuda()
    for opt in ("adam", "sgd"):
        H = make(v, dtype, transposable=True)
        W = draw_w(v, 30)
        G = draw_g(rng, n)
        if opt == "adam":
            op = tadam.Operands(n, W, G)
            step = lambda rec: H.adam_step(*op.args(), lr=1e-2, weight_decay=0.01, ctl=rec.R)      # noqa: E731
        else:
            op = tsgd.Operands(n, W, G)
            step = lambda rec: H.sgd_step(op.W, op.G, op.M, lr=0.25, momentum=0.9, ctl=rec.R)       # noqa: E731
        rec, words = control(op.G, G, dict(loss_scale=2.0))
        step(rec)                                                    # one step that counts: M, V and S hold something
        before = op.read()
        assert not same_bits(before[0], W)
        H.set_values(other)                                          # the handle holds other values than W
        Gbad = draw_g(rng, n)
        Gbad[[0, n // 2, n - 1]] = [np.inf, np.nan, -np.inf]
        op.set_grad(Gbad)
        rec, words = control(op.G, Gbad, dict(loss_scale=2.0, growth_interval=10), rec)
        r = record_fields(words)
        assert r["skip"] == 1 and float(r["coef"]) == 0.0 and r["skipped_total"] == 1 and float(r["loss_scale"]) == 1.0
        step(rec)
        after = op.read()                                            # (asserts the canaries)
        for a, b in zip(before, after):
            if a is not None:
                assert np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32)), (key, opt)
        info = H.step_info()
        assert info["launches"] >= (1 if opt == "sgd" else 2), info
        Fh = with_values(v, before[0]).to_device(0, dtype=dtype, updatable=True, transposable=True)
        assert same_bits(product(H, v, B, dtype)[0], product(Fh, v, B, dtype)[0]), (key, opt, "spmm")
        assert same_bits(run_t(H, X, dtype, v.cols)[0], run_t(Fh, X, dtype, v.cols)[0]), (key, opt, "spmm_t")
        Fh.close(); H.close()


# ---- 5. capture --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [sa.F32, sa.F16], ids=["f32", "f16"])
def test_capture_replays_through_a_nonfinite_gradient(mats, dtype, monkeypatch):
    """[grad_stats, finish, adam_step_ctl] captured once, the handle's and the record's very first calls inside the capture; G rewritten in place between the
    replays: finite, with an Inf, finite again.  Graph and eager runs agree bit for bit after every replay, and with adam_ref fed the coef read back."""
    set_fuse(monkeypatch, None)
    v = mats["padded"]
    nz = int(v.nztot)
    cfg = dict(lr=1e-2, weight_decay=0.01)
    ctl_cfg = dict(loss_scale=8.0, max_norm=1.0, growth_interval=100)
    rng = np.random.default_rng(600)
    W0 = draw_w(v, 25)
    Gs = [draw_g(rng, nz) for _ in range(3)]
    Gs[1][nz // 3] = np.inf
    out = {}
    for mode in ("eager", "graph"):
        H = make(v, dtype)
        op = tadam.Operands(nz, W0, Gs[0])
        ctl = sa.GradCtl(**ctl_cfg)
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            def step():
                ctl.add(op.G, first=True)
                ctl.finish()
                H.adam_step(*op.args(), ctl=ctl, **cfg)
            if mode == "graph":
                gph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gph, stream=s):
                    step()
                torch.cuda.synchronize()
                got = op.read()                                      # a capture runs nothing
                assert same_bits(got[0], W0) and not got[3].any() and ctl.read()["skipped_total"] == 0
            res = []
            for i in range(3):
                op.set_grad(Gs[i])
                torch.cuda.synchronize()
                gph.replay() if mode == "graph" else step()
                torch.cuda.synchronize()
                res.append(op.read() + (ctl.read(),))
        out[mode] = res
        H.close()
    ref = (W0, np.zeros(nz, f32), np.zeros(nz, f32), fresh_state())
    for i in range(3):
        e, g = out["eager"][i], out["graph"][i]
        assert np.array_equal(e[4]["words"], g[4]["words"]), (i, e[4], g[4])
        r = g[4]
        assert r["skip"] == (1 if i == 1 else 0) and r["nonfinite"] == (1 if i == 1 else 0), (i, r)
        if i != 1:
            ref = adam_ref(ref[0], scaled(Gs[i], 1.0, r["coef"]), ref[1], ref[2], ref[3], cfg)
        for mode in ("eager", "graph"):
            assert_state(out[mode][i][:4], ref, (mode, i))
    last = out["graph"][2]
    assert int(last[3][0]) == 2                                       # t advanced twice in three replays
    assert last[4]["skipped_total"] == 1 and last[4]["loss_scale"] == 4.0 and out["graph"][0][4]["loss_scale"] == 8.0


# ---- 6. end to end -----------------------------------------------------------------------------------------------------------------------------------
def train(v, dtype, x, gys, W0, loss_scale):
    """four steps of vbs_linear + VbsAdamW, with a control record (loss_scale != None) or without; returns (W after every step, G of every step)"""
    H = v.to_device(0, dtype=dtype, updatable=True, transposable=True)
    W = torch.from_numpy(W0.copy()).cuda().requires_grad_(True)
    opt = sa.VbsAdamW([(H, W)], lr=1e-2, weight_decay=0.01)
    ctl = None if loss_scale is None else sa.GradCtl(loss_scale=loss_scale)
    Ws, Gs = [], []
    for gy in gys:
        opt.zero_grad()
        y = vbs_linear(x, H, W)
        if ctl is None:
            y.backward(gy)
            opt.step()
        else:
            y.backward(gy * ctl.loss_scale)
            ctl.collect(opt)
            opt.step(ctl=ctl)
        Gs.append(W.grad.cpu().numpy().copy())
        Ws.append(W.detach().cpu().numpy().copy())
    rec = None if ctl is None else ctl.read()
    H.close()
    return Ws, Gs, rec


def test_power_of_two_loss_scale_changes_nothing_fp32(mats, monkeypatch):
    """loss_scale = 1024, no clipping, growth_interval = 0: the scale goes exactly through the products (a power of two; no |G| anywhere near overflow or
    underflow, asserted) and coef = 2^-10 takes it out exactly, so W is bit-identical to the training without a control record"""
    set_fuse(monkeypatch, None)
    v = mats["padded"]
    n = 2
    W0 = draw_w(v, 70)
    x = torch.from_numpy(np.ascontiguousarray(dense_b(v, n, 71, integer=False).T)).cuda().to(TDT[sa.F32])
    gys = [torch.from_numpy(np.ascontiguousarray(dense_x(v.rows, n, 72 + s, integer=False).T)).float().cuda() for s in range(4)]
    plain, Gp, _ = train(v, sa.F32, x, gys, W0, None)
    ctld, Gc, rec = train(v, sa.F32, x, gys, W0, 1024.0)
    assert rec["coef"] == 2.0 ** -10 and rec["skip"] == 0 and rec["skipped_total"] == 0 and rec["loss_scale"] == 1024.0
    for step in range(4):
        for G in (Gp[step], Gc[step]):
            nzv = np.abs(G[G != 0])
            assert nzv.size and nzv.max() < 2.0 ** 100 and nzv.min() > 2.0 ** -100
        assert same_bits(Gc[step], Gp[step] * f32(1024.0)), step
        assert same_bits(ctld[step], plain[step]), step
    assert not same_bits(plain[3], W0)


def test_loss_scale_rescues_an_fp16_gradient(mats, monkeypatch):
    """an fp16 handle rounds grad_y to fp16: 2^-26 flushes to zero there, so G is zero without a scale; under loss_scale = 2^16 it arrives as 2^-10, G is not
    zero and the step moves W"""
    set_fuse(monkeypatch, None)
    v = mats["padded"]
    n = 2
    W0 = draw_w(v, 73)
    x = torch.from_numpy(np.ascontiguousarray(np.sign(dense_b(v, n, 74, integer=True).T))).cuda().to(TDT[sa.F16])
    gy = torch.full((n, v.rows), 2.0 ** -26, dtype=torch.float32, device="cuda")
    _, Gp, _ = train(v, sa.F16, x, [gy], W0, None)
    assert not Gp[0].any()
    Ws, Gc, rec = train(v, sa.F16, x, [gy], W0, 2.0 ** 16)
    assert Gc[0].any() and np.all(np.isfinite(Gc[0])) and rec["skip"] == 0 and rec["coef"] == 2.0 ** -16
    moved = Ws[0] != (W0 * f32(f32(1.0) - f32(f32(1e-2) * f32(0.01))))       # beyond the weight decay alone, which both runs apply
    assert moved.any() and np.array_equal(moved, Gc[0] != 0)


# ---- 7. GradCtl and the optimizers -------------------------------------------------------------------------------------------------------------------
def test_gradctl_state_dict_round_trip():
    """state_dict() into a new GradCtl: the loss scale, the tracker and the count of skipped steps go over, coef is 1 / loss_scale until the next finish, and
    the next finish of both is grad_ctl_ref of what they held"""
    kw = dict(max_norm=1.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=3)
    G = torch.from_numpy(drawn(1000)[0].copy()).cuda()
    Gbad = G.clone()
    Gbad[5] = float("inf")
    a = sa.GradCtl(loss_scale=8.0, **kw)
    assert a.read()["coef"] == 0.125 and float(a.loss_scale) == 8.0 and a.loss_scale.dim() == 0
    a.collect([G])                                                   # a list with one gradient
    a.collect(Gbad)                                                  # a tensor alone
    a.collect([G])
    sd = a.state_dict()
    assert sd == {"loss_scale": 4.0, "growth_tracker": 1, "skipped_total": 1}
    b = sa.GradCtl(loss_scale=1.0, **kw)
    b.load_state_dict(sd)
    rb = b.read()
    assert b.state_dict() == sd and rb["coef"] == 0.25 and rb["skip"] == 0
    with pytest.raises(ValueError):
        b.load_state_dict(dict(sd, loss_scale=0.0))
    for ctl in (a, b):
        ctl.add(G, first=True)
        before = ctl.read()["words"]
        ctl.finish()
        assert np.array_equal(ctl.read()["words"], grad_ctl_ref(before, kw))
    assert a.state_dict() == b.state_dict() == {"loss_scale": 4.0, "growth_tracker": 2, "skipped_total": 1}
    assert a.read()["coef"] == b.read()["coef"] < 0.25               # clipped, from the same statistics


def test_collect_over_a_torch_optimizer_and_a_list():
    """every gradient that is present: the parameters of a torch optimizer's param_groups, a parameter on its own, a plain tensor as a gradient itself; a
    parameter without a gradient is passed over"""
    parts = [drawn(1000)[0].copy(), drawn(CHUNK + 1)[0].copy(), drawn(257)[0].copy(), drawn(13, seed=1)[0].copy()]
    parts[1][7] = np.nan
    params = [torch.zeros(len(p), device="cuda", requires_grad=True) for p in parts[:3]]
    for p, g in zip(params, parts[:3]):
        p.grad = torch.from_numpy(g).cuda()
    idle = torch.zeros(50, device="cuda", requires_grad=True)        # no gradient
    opt = torch.optim.SGD([{"params": [params[0], idle]}, {"params": [params[1]]}], lr=0.1)
    raw = torch.from_numpy(parts[3]).cuda()
    ctl = sa.GradCtl()
    ctl.collect([opt, params[2], raw])
    r = ctl.read()
    want, k = stats_ref(np.concatenate(parts))
    assert r["nonfinite"] == k == 1 and r["skip"] == 1 and within(r["ssq"], want, sum(len(p) for p in parts)), (r, want)
    ctl.collect(torch.optim.SGD([params[0], idle], lr=0.1))          # an optimizer alone; the statistics start over
    r = ctl.read()
    want, _ = stats_ref(parts[0])
    assert r["nonfinite"] == 0 and r["skip"] == 0 and r["skipped_total"] == 1 and within(r["ssq"], want, len(parts[0])), (r, want)
    ctl.collect([idle])                                              # nothing present: zeros
    r = ctl.read()
    assert r["ssq"] == 0.0 and r["nonfinite"] == 0 and r["norm"] == 0.0 and r["coef"] == 1.0
    with pytest.raises(ValueError):
        ctl.add(raw.double())


def test_vbs_sgd_step_under_control(mats, monkeypatch):
    """VbsSGD.step(ctl=): clipped and unscaled by the record, then skipped on a gradient with an Inf"""
    set_fuse(monkeypatch, None)
    v = mats["padded"]
    n = int(v.nztot)
    rng = np.random.default_rng(700)
    H = make(v, sa.F32)
    W0 = draw_w(v, 80)
    W = torch.from_numpy(W0.copy()).cuda().requires_grad_(True)
    opt = sa.VbsSGD([(H, W)], lr=0.25, momentum=0.9)
    ctl = sa.GradCtl(loss_scale=4.0, max_norm=1.0)
    Wr, M = W0, np.zeros(n, f32)
    for step in range(2):
        G = draw_g(rng, n)
        W.grad = torch.from_numpy(G).cuda()
        ctl.collect(opt)
        opt.step(ctl=ctl)
        r = ctl.read()
        assert r["skip"] == 0 and 0 < r["coef"] < 0.25
        Wr, M = sgd_ref(Wr, scaled(G, 1.0, f32(r["coef"])), M, 0.25, 0.9)
        assert same_bits(W.detach().cpu().numpy(), Wr), step
    G[n // 2] = np.inf
    W.grad = torch.from_numpy(G).cuda()
    ctl.collect(opt)
    opt.step(ctl=ctl)
    assert ctl.read()["skip"] == 1 and ctl.state_dict()["skipped_total"] == 1
    assert same_bits(W.detach().cpu().numpy(), Wr)
    H.close()
