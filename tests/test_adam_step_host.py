"""sparta_vbs_adam_step (Adam / AdamW and set_values in one pass, k_update.hip) without a GPU: adam_ref, the numpy float32 restatement of the arithmetic
include/sparta_amd.h pins (tests/test_adam_step_gpu.py holds the kernels to it bit for bit), is as close to torch.optim.AdamW / Adam in float64 as torch's
own float32 run is; the entry is exported with the declared prototype; a NULL handle is refused with a message that names the entry; the eleven kernels of
the step keep their state in registers; sparta_amd.optim does not import torch on its own."""
import ctypes as C
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
TINY = np.finfo(f32).tiny


def _f(x):
    """an intermediate of adam_ref: float32, or the restatement is not one"""
    assert isinstance(x, (np.ndarray, np.generic)) and x.dtype == f32, getattr(x, "dtype", type(x))
    return x


def fresh_state():
    return np.zeros(8, np.uint32)


def adam_ref(W, G, M, V, S, cfg):
    """The arithmetic of sparta_vbs_adam_step in numpy float32: one rounding per operation, no fused multiply-add, division and square root correctly
    rounded.  W, G, M, V: float32 arrays; S: the 8-word step state (uint32 words; zeros = a fresh optimizer); cfg: dict(lr, betas=(0.9, 0.999), eps=1e-8,
    weight_decay=0, decoupled=True, grad_scale=1).  Returns (W, M, V, S) after the step; the inputs are left as they are."""
    lr, (beta1, beta2), eps = f32(cfg["lr"]), (f32(b) for b in cfg.get("betas", (0.9, 0.999))), f32(cfg.get("eps", 1e-8))
    wd, gs, decoupled = f32(cfg.get("weight_decay", 0.0)), f32(cfg.get("grad_scale", 1.0)), bool(cfg.get("decoupled", True))
    one = f32(1.0)
    S = np.array(S).view(np.uint32).copy()
    assert S.shape == (8,)
    t, p1, p2 = int(S[0:1].view(np.int32)[0]), S[1:2].view(f32)[0], S[2:3].view(f32)[0]
    # once per step
    if t == 0:
        p1, p2 = beta1, beta2
    else:
        p1, p2 = _f(p1 * beta1), _f(p2 * beta2)
    t = t + 1
    bc1, bc2 = _f(one - p1), _f(one - p2)
    step_size, d = _f(lr / bc1), _f(np.sqrt(bc2))
    S[0:1].view(np.int32)[0] = t
    S[1:5].view(f32)[:] = (p1, p2, step_size, d)
    S[5:] = 0
    # per element
    omb1, omb2, dk = _f(one - beta1), _f(one - beta2), _f(one - _f(lr * wd))
    W, g, M, V = (np.asarray(a) for a in (W, G, M, V))
    for a in (W, g, M, V):
        _f(a)
    if gs != 1:
        g = _f(g * gs)
    w = W
    if wd != 0 and decoupled:
        w = _f(W * dk)
    if wd != 0 and not decoupled:
        g = _f(g + _f(wd * w))
    m = _f(_f(beta1 * M) + _f(omb1 * g))
    v = _f(_f(beta2 * V) + _f(omb2 * _f(g * g)))
    den = _f(_f(_f(np.sqrt(v)) / d) + eps)
    Wn = _f(w - _f(step_size * _f(m / den)))
    return Wn, m, v, S


def state_fields(S):
    S = np.asarray(S).view(np.uint32)
    return int(S[0:1].view(np.int32)[0]), [float(x) for x in S[1:5].view(f32)], [int(x) for x in S[5:]]


def test_adam_ref_state_words():
    """the once-per-step block: t counts, the running products are products, step_size and d follow, words 5..7 are zero"""
    S = fresh_state()
    z = np.zeros(3, f32)
    cfg = dict(lr=1e-2)
    for step in range(1, 5):
        _, _, _, S = adam_ref(z, z, z, z, S, cfg)
        t, (p1, p2, step_size, d), rest = state_fields(S)
        assert t == step and rest == [0, 0, 0]
        assert abs(p1 - 0.9 ** step) < 1e-6 and abs(p2 - 0.999 ** step) < 1e-6
        # bc = 1 - p carries p's absolute error (< step * 2^-23, the roundings of beta and of the products) into a small number: relative step * 2^-23 / bc
        assert abs(step_size - 1e-2 / (1 - 0.9 ** step)) < step_size * (step * 2.0 ** -23 / (1 - 0.9 ** step) + 2.0 ** -22)
        assert abs(d - (1 - 0.999 ** step) ** 0.5) < step * 2.0 ** -23 / (2 * d) + d * 2.0 ** -23


@pytest.mark.parametrize("weight_decay", [0.0, 0.01], ids=["wd0", "wd0.01"])
@pytest.mark.parametrize("decoupled", [1, 0], ids=["adamw", "adam"])
def test_adam_ref_is_as_close_to_torch_float64_as_torch_float32(decoupled, weight_decay):
    """six steps on n = 20 000 elements, |W|, |G| in {0} u [2^-8, 4], a fifth of G zero, lr = 1e-2, default betas and eps: the distance of adam_ref to
    torch.optim.AdamW / Adam run in float64 is at most twice the distance of torch's own float32 run to it (both computed here, after every step: the bound
    calibrates itself), and no non-zero M or V on the way is subnormal (so flush-to-zero could not be told from gradual underflow on these inputs -- the
    kernels keep denormals; the GPU test draws its inputs the same way)."""
    torch = pytest.importorskip("torch")
    from test_sgd_step_gpu import away_from_denormals
    n, lr = 20000, 1e-2
    rng = np.random.default_rng(1234)
    W0 = away_from_denormals(rng.uniform(-4, 4, n) * (rng.random(n) < 0.9))
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    params = {dt: torch.from_numpy(W0.copy()).to(dt).requires_grad_(True) for dt in (torch.float64, torch.float32)}
    opts = {dt: cls([p], lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=weight_decay) for dt, p in params.items()}
    cfg = dict(lr=lr, weight_decay=weight_decay, decoupled=bool(decoupled))
    W, M, V, S = W0, np.zeros(n, f32), np.zeros(n, f32), fresh_state()
    worst_ref = worst_t32 = 0.0
    for step in range(6):
        G = away_from_denormals(rng.uniform(-4, 4, n) * (rng.random(n) < 0.8))
        assert 0.1 < (G == 0).mean() < 0.3
        for dt, p in params.items():
            p.grad = torch.from_numpy(G.copy()).to(dt)
            opts[dt].step()
        W, M, V, S = adam_ref(W, G, M, V, S, cfg)
        for x in (M, V):
            nz = np.abs(x[x != 0])
            assert nz.size and nz.min() >= TINY, (step, float(nz.min()))
        t64 = params[torch.float64].detach().numpy()
        e_ref = float(np.abs(W.astype(np.float64) - t64).max())
        e_t32 = float(np.abs(params[torch.float32].detach().numpy().astype(np.float64) - t64).max())
        print("step %d: |ref - torch64| = %.3e   |torch32 - torch64| = %.3e" % (step, e_ref, e_t32))
        worst_ref, worst_t32 = max(worst_ref, e_ref), max(worst_t32, e_t32)
        assert e_ref <= 2 * e_t32, (step, e_ref, e_t32)
    assert state_fields(S)[0] == 6
    assert 0 < worst_ref <= 2 * worst_t32


def test_adam_step_symbol_and_prototype():
    assert "sparta_vbs_adam_step" in _lib.SYMBOLS and hasattr(lib, "sparta_vbs_adam_step")
    f32p, vp = C.POINTER(C.c_float), C.c_void_p
    assert list(lib.sparta_vbs_adam_step.argtypes) == [vp, f32p, f32p, f32p, f32p, vp, C.POINTER(_lib.AdamCfg), vp, f32p]
    assert [(n, t) for n, t in _lib.AdamCfg._fields_] == ([(n, C.c_float) for n in ("lr", "beta1", "beta2", "eps", "weight_decay", "grad_scale")]
                                                           + [("decoupled", C.c_int32), ("reserved", C.c_int32)])
    assert C.sizeof(_lib.AdamCfg) == 32
    hdr = open(os.path.join(ROOT, "include", "sparta_amd.h")).read()
    assert ("typedef struct sparta_adam_cfg { float lr, beta1, beta2, eps, weight_decay, grad_scale; int32_t decoupled; int32_t reserved; } sparta_adam_cfg;"
            in hdr)
    assert ("int sparta_vbs_adam_step(sparta_vbs_t* A, float* W, const float* G, float* M, float* V, void* S,\n"
            "                         const sparta_adam_cfg* cfg, void* stream, float* dt_ms);" in hdr)
    assert "int sparta_vbs_step_info(const sparta_vbs_t* A, int64_t* info_out);" in hdr           # (its prototype does not change)


def test_adam_step_null_handle_is_invalid():
    a = [(C.c_float * 4)() for _ in range(4)]
    S = (C.c_int32 * 8)()
    cfg = _lib.AdamCfg(1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, 1, 0)
    rc = lib.sparta_vbs_adam_step(None, a[0], a[1], a[2], a[3], S, C.byref(cfg), None, None)
    assert rc == _lib.ERR_INVALID
    msg = lib.sparta_last_error().decode()
    assert "sparta_vbs_adam_step" in msg and "NULL" in msg, msg
    assert list(S) == [0] * 8


def test_adam_kernels_registers_only(tmp_path):
    kernels = _kernel_metadata(tmp_path)
    adam = {n: m for n, m in kernels.items() if "vbs_adam_" in n}
    # the tick, the elementwise kernel, the fp32 fragment kernel, and the 16-bit stream-slice kernel for {f16, bf16} x {32x32, 64x32, 32x64, 64x64 slices}
    assert len(adam) == 11, sorted(adam)
    for part, count in (("vbs_adam_tick_kernel", 1), ("vbs_adam_step_kernel", 1), ("vbs_adam_f32_frag_kernel", 1), ("vbs_adam_h16_kernel", 8)):
        assert sum(part in n for n in adam) == count, (part, sorted(adam))
    for name, m in adam.items():
        assert m["private_segment_fixed_size"] == 0, (name, m)
        assert m["vgpr_spill_count"] == 0, (name, m)
        assert not any(p in name for p in ("vbs_sgd_", "vbs_update_", "stream_kernel", "direct_kernel", "sddmm")), name  # (other tests count kernels by these)


def test_optim_with_adamw_imports_without_torch():
    """sparta_amd.optim in a process where `import torch` fails: the module loads, a VbsAdamW can be made and zero_grad() called (torch is needed by step()
    and the state only)"""
    code = ("import sys; sys.modules['torch'] = None\n"
            "import sparta_amd.optim as o, sparta_amd as sa\n"
            "opt = sa.VbsAdamW([], lr=1e-3)\n"
            "opt.zero_grad()\n"
            "opt.step()\n"
            "assert o.VbsAdamW is sa.VbsAdamW and sys.modules.get('torch') is None\n"
            "print('ok')\n")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.stdout, r.stderr)
    src = open(os.path.join(ROOT, "sparta_amd", "optim.py")).read()
    assert not [ln for ln in src.splitlines() if ln.startswith(("import torch", "from torch"))]
