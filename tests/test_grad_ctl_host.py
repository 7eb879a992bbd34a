"""sparta_grad_stats / sparta_grad_ctl_finish / sparta_vbs_*_step_ctl (k_gradctl.hip, k_update.hip) without a GPU: stats_ref and grad_ctl_ref, the numpy
restatement of the arithmetic include/sparta_amd.h pins (tests/test_grad_ctl_gpu.py holds the kernels to it bit for bit), give clip_grad_norm_'s coefficient
and GradScaler.update()'s rule; the entries are exported with the declared prototypes; NULL and misaligned records are refused with a message that names
the entry; the three kernels keep their state in registers; sparta_amd.optim and GradCtl import without torch."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import sparta_amd  # noqa: F401  (loads the library)
from sparta_amd import _lib
from sparta_amd._lib import lib

from test_code_object import _kernel_metadata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
U = 2.0 ** -24                                                       # one fp32 rounding, relative


def _f(x):
    """an intermediate of grad_ctl_ref: float32, or the restatement is not one"""
    assert isinstance(x, (np.ndarray, np.generic)) and x.dtype == f32, getattr(x, "dtype", type(x))
    return x


def stats_ref(G):
    """(ssq, nonfinite) of sparta_grad_stats: the exactly rounded sum (math.fsum) of the exact fp64 squares of the finite elements -- 24-bit significands:
    a square has 48 bits and fits a double -- and the number of the others"""
    G = np.asarray(G)
    assert G.dtype == f32
    finite = np.isfinite(G)
    sq = G[finite].astype(np.float64)
    sq = sq * sq
    return math.fsum(sq.tolist()), int((~finite).sum())


def fresh_record(loss_scale=None, ssq=0.0, nonfinite=0, growth_tracker=0, skipped_total=0):
    """the 16 words of a record; loss_scale=None leaves word 4 zero (which means 1.0f)"""
    w = np.zeros(16, np.uint32)
    w[0:2].view(np.float64)[0] = ssq
    w[2:3].view(np.int32)[0] = nonfinite
    if loss_scale is not None:
        w[4:5].view(f32)[0] = loss_scale
    w[5:6].view(np.int32)[0] = growth_tracker
    w[9:10].view(np.int32)[0] = skipped_total
    return w


def record_fields(w):
    w = np.asarray(w).view(np.uint32)
    return {"ssq": float(w[0:2].view(np.float64)[0]), "nonfinite": int(w[2:3].view(np.int32)[0]), "loss_scale": w[4:5].view(f32)[0],
            "growth_tracker": int(w[5:6].view(np.int32)[0]), "norm": w[6:7].view(f32)[0], "coef": w[7:8].view(f32)[0], "skip": int(w[8]),
            "skipped_total": int(w[9:10].view(np.int32)[0])}


def grad_ctl_ref(record, cfg):
    """The arithmetic of sparta_grad_ctl_finish in numpy float32: one rounding per operation, no fused multiply-add, division and square root correctly
    rounded.  record: the 16 words (uint32); cfg: dict(max_norm=0, growth_factor=2, backoff_factor=0.5, growth_interval=0).  Returns the 16 words after
    the call; the input is left as it is."""
    max_norm, growth, backoff = (f32(cfg.get(k, d)) for k, d in (("max_norm", 0.0), ("growth_factor", 2.0), ("backoff_factor", 0.5)))
    interval = int(cfg.get("growth_interval", 0))
    w = np.array(record).view(np.uint32).copy()
    assert w.shape == (16,)
    ssq, nonfinite = w[0:2].view(np.float64)[0], int(w[2:3].view(np.int32)[0])
    s = f32(1.0) if w[4] == 0 else w[4:5].view(f32)[0]
    tracker, skipped = int(w[5:6].view(np.int32)[0]), int(w[9:10].view(np.int32)[0])
    one = f32(1.0)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        inv = _f(one / s)
        bad = nonfinite != 0
        root = _f(f32(np.sqrt(np.float64(ssq))))                     # fp64 square root, then rounded to fp32 (may be +Inf)
        norm = _f(root * inv)
        if not np.isfinite(norm):
            bad = True
        coef = inv
        if not bad and max_norm > 0:
            c = _f(max_norm / _f(norm + f32(1e-6)))
            if c < one:
                coef = _f(inv * c)
        if bad:
            coef = f32(0.0)
        skip = 1 if bad else 0
        skipped += skip
        if interval > 0:
            if skip:
                s = _f(s * backoff)
                tracker = 0
            else:
                tracker += 1
                if tracker >= interval:
                    s2 = _f(s * growth)
                    if np.isfinite(s2):
                        s = s2
                    tracker = 0
    w[4:5].view(f32)[0] = s
    w[5:6].view(np.int32)[0] = tracker
    w[6:7].view(f32)[0] = norm
    w[7:8].view(f32)[0] = coef
    w[8] = skip
    w[9:10].view(np.int32)[0] = skipped
    w[10:] = 0
    return w


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------------------
def test_stats_ref_counts_and_sums():
    G = np.array([3.0, -4.0, np.inf, 0.0, np.nan, -np.inf, 1e-40, 2.0 ** 60], f32)
    ssq, bad = stats_ref(G)
    assert bad == 3
    assert ssq == math.fsum([9.0, 16.0, float(f32(1e-40)) ** 2, 2.0 ** 120])
    assert stats_ref(np.zeros(0, f32)) == (0.0, 0)


@pytest.mark.parametrize("loss_scale", [1.0, 1024.0, 3.0], ids=["s1", "s1024", "s3"])
@pytest.mark.parametrize("max_norm", [0.5, 1.0, 1e4], ids=["clip0.5", "clip1", "inactive"])
def test_coef_is_clip_grad_norm_in_float64(max_norm, loss_scale):
    """coef * s against the coefficient torch.nn.utils.clip_grad_norm_ applies to the UNSCALED gradient in float64 (read off as grad_after / grad_before at the
    largest element).  The bound, in units of u = 2^-24, counts the fp32 roundings on the way from the exact quantities to coef * s (the product itself is
    taken in float64 here):
        inv = fl(1 / s)                      1      root = fl32(sqrt(ssq))          1   (the fp64 square root and fsum add ~2^-53: nothing)
        norm = fl(root * inv)                1      norm + fl32(1e-6)               2   (the constant's own rounding, at most its share of the sum; the add)
        c = fl(max_norm / ...)               1      coef = fl(inv * c)              1
        inv * s = 1 +- u, in coef * s        1
    -- 8 roundings, each a factor (1 +- u): |coef * s / c64 - 1| <= (1 + u)^8 - 1 < 9 u.  torch's own float64 arithmetic (norm, + 1e-6, the division, the
    multiplication we divide back out) adds a few 2^-53.  max_norm is exact in fp32 in all three cases.  Where the clip is inactive torch clamps to 1 and
    coef * s = inv * s: one rounding."""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(77)
    n = 5000
    G = (rng.uniform(-4, 4, n) * (rng.random(n) < 0.8)).astype(f32)         # the scaled gradient, as the backward leaves it
    assert float(f32(max_norm)) == max_norm
    p = torch.zeros(n, dtype=torch.float64, requires_grad=True)
    p.grad = torch.from_numpy(G.astype(np.float64)) / loss_scale
    before = p.grad.clone()
    total = float(torch.nn.utils.clip_grad_norm_([p], max_norm))
    k = int(before.abs().argmax())
    c64 = float(p.grad[k] / before[k])
    ssq, bad = stats_ref(G)
    assert bad == 0 and abs(math.sqrt(ssq) / loss_scale - total) <= 1e-12 * total
    out = record_fields(grad_ctl_ref(fresh_record(loss_scale, ssq), dict(max_norm=max_norm)))
    assert out["skip"] == 0 and abs(float(out["norm"]) - total) <= 3 * U * total
    got = float(out["coef"]) * loss_scale
    print("max_norm %g, s %g: norm %.9g, coef * s = %.9g, torch float64 %.9g" % (max_norm, loss_scale, total, got, c64))
    assert (c64 < 1.0) == (total > max_norm)
    assert abs(got / c64 - 1.0) <= 9 * U + 1e-14


def test_loss_scale_follows_the_rule():
    """a hand-written sequence against GradScaler.update()'s rule (and against torch._amp_update_scale_ itself where this torch runs it on the CPU): growth
    after `growth_interval` finite steps in a row, backoff and a reset tracker on a non-finite one, a growth that would overflow refused"""
    cfg = dict(growth_factor=2.0, backoff_factor=0.5, growth_interval=2)
    seq = [(False, 65536.0, 1), (False, 131072.0, 0), (True, 65536.0, 0), (False, 65536.0, 1), (True, 32768.0, 0), (False, 32768.0, 1),
           (False, 65536.0, 0), (False, 65536.0, 1)]
    w = fresh_record(65536.0)
    try:
        import torch
        ts, tt = torch.full((1,), 65536.0), torch.zeros(1, dtype=torch.int32)
        torch._amp_update_scale_(ts.clone(), tt.clone(), torch.zeros(1), 2.0, 0.5, 2)
    except (ImportError, NotImplementedError, RuntimeError):         # no torch, or no CPU kernel for the op: the hand-written column stands alone
        ts = None
    skipped = 0
    for i, (overflow, want_s, want_t) in enumerate(seq):
        w[0:2].view(np.float64)[0] = 25.0
        w[2] = 4 if overflow else 0
        w = grad_ctl_ref(w, cfg)
        r = record_fields(w)
        skipped += overflow
        assert (float(r["loss_scale"]), r["growth_tracker"], r["skip"], r["skipped_total"]) == (want_s, want_t, int(overflow), skipped), (i, r)
        assert float(r["coef"]) == (0.0 if overflow else 1.0 / seq[i - 1][1] if i else 1.0 / 65536.0), (i, r)     # the scale the gradients were produced under
        if ts is not None:
            torch._amp_update_scale_(ts, tt, torch.full((1,), float(overflow)), 2.0, 0.5, 2)
            assert (float(ts), int(tt)) == (want_s, want_t), i
    # s * growth_factor overflows: the scale stays, the tracker starts over
    w = grad_ctl_ref(fresh_record(2.0 ** 127, 1.0, growth_tracker=1), cfg)
    r = record_fields(w)
    assert (float(r["loss_scale"]), r["growth_tracker"], r["skip"]) == (2.0 ** 127, 0, 0)
    # growth_interval = 0: nothing moves
    r = record_fields(grad_ctl_ref(fresh_record(8.0, 1.0, nonfinite=1, growth_tracker=3), dict(growth_interval=0)))
    assert (float(r["loss_scale"]), r["growth_tracker"], r["skip"], float(r["coef"])) == (8.0, 3, 1, 0.0)


def test_grad_ctl_ref_edges():
    """a zero loss-scale word is 1.0f; a norm that overflows fp32 skips (with a loss scale below 1 a finite root can do it); max_norm = 0 never clips; the
    words behind skipped_total come back zero"""
    w = fresh_record(None, 9.0)
    w[10:] = 0xdeadbeef
    out = grad_ctl_ref(w, dict(max_norm=1.0))
    r = record_fields(out)
    assert (float(r["loss_scale"]), float(r["norm"]), r["skip"]) == (1.0, 3.0, 0) and not out[10:].any()
    assert float(r["coef"]) == float(f32(1.0) / (f32(3.0) + f32(1e-6)))
    r = record_fields(grad_ctl_ref(fresh_record(0.25, 9e76), {}))
    assert np.isinf(r["norm"]) and r["skip"] == 1 and float(r["coef"]) == 0.0
    r = record_fields(grad_ctl_ref(fresh_record(1.0, 1e80), {}))
    assert np.isinf(r["norm"]) and r["skip"] == 1
    r = record_fields(grad_ctl_ref(fresh_record(4.0, 1e30), dict(max_norm=0.0)))
    assert r["skip"] == 0 and float(r["coef"]) == 0.25


# ---- the ABI -----------------------------------------------------------------------------------------------------------------------------------------
def test_symbols_and_prototypes():
    f32p, vp = C.POINTER(C.c_float), C.c_void_p
    for name in ("sparta_grad_stats", "sparta_grad_ctl_finish", "sparta_vbs_sgd_step_ctl", "sparta_vbs_adam_step_ctl"):
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    assert list(lib.sparta_grad_stats.argtypes) == [f32p, C.c_int64, vp, C.c_int32, vp, f32p]
    assert list(lib.sparta_grad_ctl_finish.argtypes) == [vp, C.POINTER(_lib.GradCtlCfg), vp]
    assert list(lib.sparta_vbs_sgd_step_ctl.argtypes) == [vp, f32p, f32p, f32p, C.POINTER(_lib.SgdCfg), vp, vp, f32p]
    assert list(lib.sparta_vbs_adam_step_ctl.argtypes) == [vp, f32p, f32p, f32p, f32p, vp, C.POINTER(_lib.AdamCfg), vp, vp, f32p]
    assert [(n, t) for n, t in _lib.GradCtlCfg._fields_[:4]] == [("max_norm", C.c_float), ("growth_factor", C.c_float), ("backoff_factor", C.c_float),
                                                                 ("growth_interval", C.c_int32)]
    assert C.sizeof(_lib.GradCtlCfg) == 32
    hdr = open(os.path.join(ROOT, "include", "sparta_amd.h")).read()
    for text in ("typedef struct sparta_grad_ctl_cfg {\n    float max_norm, growth_factor, backoff_factor;\n    int32_t growth_interval;\n"
                 "    int32_t reserved[4];\n} sparta_grad_ctl_cfg;",
                 "int sparta_grad_stats(const float* G, int64_t n, void* R, int32_t accumulate, void* stream, float* dt_ms);",
                 "int sparta_grad_ctl_finish(void* R, const sparta_grad_ctl_cfg* cfg, void* stream);",
                 "int sparta_vbs_sgd_step_ctl(sparta_vbs_t* A, float* W, const float* G, float* M, const sparta_sgd_cfg* cfg, const void* R, void* stream, "
                 "float* dt_ms);",
                 "int sparta_vbs_adam_step_ctl(sparta_vbs_t* A, float* W, const float* G, float* M, float* V, void* S,\n"
                 "                             const sparta_adam_cfg* cfg, const void* R, void* stream, float* dt_ms);",
                 "#define SPARTA_GRAD_CTL_BYTES %d\n" % _lib.GRAD_CTL_BYTES,
                 "#define SPARTA_GRAD_STATS_CHUNK %d\n" % _lib.GRAD_STATS_CHUNK,
                 "#define SPARTA_GRAD_STATS_MAX_GRID %d\n" % _lib.GRAD_STATS_MAX_GRID):
        assert text in hdr, text
    # the record: 64 bytes + one 16-byte partial per workgroup of the largest grid; 8-byte granular
    assert _lib.GRAD_CTL_BYTES == 64 + 16 * _lib.GRAD_STATS_MAX_GRID and _lib.GRAD_CTL_BYTES % 8 == 0


def test_null_and_misaligned_records_are_refused():
    """every refusal comes before anything touches the device: the pointers below are never dereferenced"""
    aligned, off4 = C.c_void_p(0x10000), C.c_void_p(0x10004)
    g = (C.c_float * 4)()
    cfg = _lib.GradCtlCfg(1.0, 2.0, 0.5, 0, (C.c_int32 * 4)())

    def refused(rc, entry, word):
        msg = lib.sparta_last_error().decode()
        assert rc == _lib.ERR_INVALID and entry in msg and word in msg, (rc, msg)

    refused(lib.sparta_grad_stats(g, 4, None, 0, None, None), "sparta_grad_stats", "NULL")
    refused(lib.sparta_grad_stats(g, 4, off4, 0, None, None), "sparta_grad_stats", "8-byte")
    refused(lib.sparta_grad_stats(None, 4, aligned, 0, None, None), "sparta_grad_stats", "NULL")
    refused(lib.sparta_grad_stats(g, -1, aligned, 0, None, None), "sparta_grad_stats", "n < 0")
    refused(lib.sparta_grad_ctl_finish(None, C.byref(cfg), None), "sparta_grad_ctl_finish", "NULL")
    refused(lib.sparta_grad_ctl_finish(aligned, None, None), "sparta_grad_ctl_finish", "NULL")
    refused(lib.sparta_grad_ctl_finish(off4, C.byref(cfg), None), "sparta_grad_ctl_finish", "8-byte")
    for bad, word in ((_lib.GradCtlCfg(-1.0, 2.0, 0.5, 0), "max_norm"), (_lib.GradCtlCfg(float("nan"), 2.0, 0.5, 0), "max_norm"),
                      (_lib.GradCtlCfg(1.0, 0.5, 0.5, 10), "growth_factor"), (_lib.GradCtlCfg(1.0, 2.0, 0.0, 10), "backoff_factor"),
                      (_lib.GradCtlCfg(1.0, 2.0, 1.5, 10), "backoff_factor"), (_lib.GradCtlCfg(1.0, 2.0, 0.5, -1), "growth_interval"),
                      (_lib.GradCtlCfg(1.0, 2.0, 0.5, 0, (C.c_int32 * 4)(0, 0, 7, 0)), "reserved")):
        refused(lib.sparta_grad_ctl_finish(aligned, C.byref(bad), None), "sparta_grad_ctl_finish", word)
    # the steps: a NULL handle is named by the entry that was called
    a = [(C.c_float * 4)() for _ in range(4)]
    S = (C.c_int32 * 8)()
    refused(lib.sparta_vbs_adam_step_ctl(None, a[0], a[1], a[2], a[3], S, C.byref(_lib.AdamCfg(1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, 1, 0)), aligned, None, None),
            "sparta_vbs_adam_step_ctl", "NULL handle")
    refused(lib.sparta_vbs_sgd_step_ctl(None, a[0], a[1], a[2], C.byref(_lib.SgdCfg(0.5, 0.0, 0.0, 1.0)), aligned, None, None),
            "sparta_vbs_sgd_step_ctl", "NULL handle")
    assert list(S) == [0] * 8


# ---- the kernels -------------------------------------------------------------------------------------------------------------------------------------
def test_gradctl_kernels_registers_only(tmp_path):
    kernels = _kernel_metadata(tmp_path)
    ctl = {n: m for n, m in kernels.items() if "vbs_gradctl_" in n}
    assert len(ctl) == 3, sorted(ctl)
    for part in ("vbs_gradctl_stats_kernel", "vbs_gradctl_fold_kernel", "vbs_gradctl_finish_kernel"):
        assert sum(part in n for n in ctl) == 1, (part, sorted(ctl))
    for name, m in ctl.items():
        assert m["private_segment_fixed_size"] == 0, (name, m)
        assert m["vgpr_spill_count"] == 0, (name, m)
        assert not any(p in name for p in ("vbs_adam_", "vbs_sgd_", "vbs_update_", "stream_kernel", "direct_kernel", "sddmm")), name   # (other tests count kernels by these)


# ---- imports -----------------------------------------------------------------------------------------------------------------------------------------
def test_grad_ctl_imports_without_torch():
    """sparta_amd with GradCtl in a process where `import torch` fails: the modules load, VbsAdamW.step takes the new argument (torch is needed to make a
    GradCtl, not to import it)"""
    code = ("import sys; sys.modules['torch'] = None\n"
            "import sparta_amd.optim as o, sparta_amd.gradctl as g, sparta_amd as sa\n"
            "assert sa.GradCtl is g.GradCtl and sa._lib.GRAD_CTL_BYTES == 16448\n"
            "sa.VbsAdamW([], lr=1e-3).step(ctl=None)\n"
            "try:\n"
            "    sa.GradCtl()\n"
            "except ImportError:\n"
            "    print('ok')\n")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.stdout, r.stderr)
    for mod in ("optim.py", "gradctl.py"):
        src = open(os.path.join(ROOT, "sparta_amd", mod)).read()
        assert not [ln for ln in src.splitlines() if ln.startswith(("import torch", "from torch"))], mod
