"""sparta_vbs_sgd_step / sparta_vbs_step_info (the optimizer step and set_values in one pass, k_update.hip) without a GPU: the entries are exported with
the declared prototypes, a NULL handle is refused with a message that names the entry, the kernels of the step keep their state in registers and
contain no fused multiply-add (the arithmetic is pinned operation by operation), the kernels of set_values are the ones it had, and sparta_amd.optim
does not import torch on its own."""
import ctypes as C
import os
import subprocess
import sys

import sparta_amd  # noqa: F401  (loads the library)
from sparta_amd import _lib
from sparta_amd._lib import lib

from test_code_object import _kernel_metadata, _disassemble

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sgd_step_symbols_and_prototypes():
    for s in ("sparta_vbs_sgd_step", "sparta_vbs_step_info"):
        assert s in _lib.SYMBOLS, s
        assert hasattr(lib, s), s
    f32p, i64p, vp = C.POINTER(C.c_float), C.POINTER(C.c_int64), C.c_void_p
    assert list(lib.sparta_vbs_sgd_step.argtypes) == [vp, f32p, f32p, f32p, C.POINTER(_lib.SgdCfg), vp, f32p]
    assert list(lib.sparta_vbs_step_info.argtypes) == [vp, i64p]
    assert [(n, t) for n, t in _lib.SgdCfg._fields_] == [(n, C.c_float) for n in ("lr", "momentum", "weight_decay", "grad_scale")]
    assert C.sizeof(_lib.SgdCfg) == 16
    hdr = open(os.path.join(ROOT, "include", "sparta_amd.h")).read()
    assert "typedef struct sparta_sgd_cfg { float lr, momentum, weight_decay, grad_scale; } sparta_sgd_cfg;" in hdr
    assert ("int sparta_vbs_sgd_step(sparta_vbs_t* A, float* W, const float* G, float* M, const sparta_sgd_cfg* cfg, void* stream, float* dt_ms);"
            in hdr)
    assert "int sparta_vbs_step_info(const sparta_vbs_t* A, int64_t* info_out);" in hdr


def test_sgd_step_null_handle_is_invalid():
    w, g = (C.c_float * 4)(), (C.c_float * 4)()
    cfg = _lib.SgdCfg(0.5, 0.0, 0.0, 1.0)
    rc = lib.sparta_vbs_sgd_step(None, w, g, None, C.byref(cfg), None, None)
    assert rc == _lib.ERR_INVALID
    msg = lib.sparta_last_error().decode()
    assert "sparta_vbs_sgd_step" in msg and "NULL" in msg, msg
    out = (C.c_int64 * 4)(7, 7, 7, 7)
    assert lib.sparta_vbs_step_info(None, out) == _lib.ERR_INVALID
    assert "sparta_vbs_step_info" in lib.sparta_last_error().decode()
    assert list(out) == [7, 7, 7, 7]


def test_sgd_kernels_registers_only_and_no_fma(tmp_path):
    kernels = _kernel_metadata(tmp_path)
    sgd = {n: m for n, m in kernels.items() if "vbs_sgd_" in n}
    # the elementwise kernel, the fp32 fragment kernel, and the 16-bit stream-slice kernel for {f16, bf16} x {32x32, 64x32, 32x64, 64x64 slices}
    assert len(sgd) == 10, sorted(sgd)
    assert sum("vbs_sgd_step_kernel" in n for n in sgd) == 1 and sum("vbs_sgd_f32_frag_kernel" in n for n in sgd) == 1
    assert sum("vbs_sgd_h16_kernel" in n for n in sgd) == 8
    for name, m in sgd.items():
        assert m["private_segment_fixed_size"] == 0, (name, m)
        assert m["vgpr_spill_count"] == 0, (name, m)
        assert not any(p in name for p in ("stream_kernel", "direct_kernel", "sddmm", "vbs_update_")), name    # (other tests count kernels by these patterns)
    txt = {n: t for n, t in _disassemble(tmp_path).items() if "vbs_sgd_" in n}
    assert len(txt) == 10, sorted(txt)
    fused = ("v_fma_f32", "v_fmac_f32", "v_mac_f32", "v_mad_f32", "v_pk_fma_f32", "v_fma_mix", "v_mad_legacy_f32", "v_fma_legacy_f32")
    for name, t in txt.items():
        ins = [ln.split()[0] for ln in t.splitlines() if ln.strip()]
        assert any(i.startswith("v_mul_f32") or i.startswith("v_pk_mul_f32") for i in ins), name               # (the arithmetic is there ...)
        assert not [i for i in ins if i.startswith(fused)], name                                                # (... one rounding per operation)


def test_optim_imports_without_torch():
    """sparta_amd.optim in a process where `import torch` fails: the module loads and an optimizer can be made (torch is needed by step() only)"""
    code = ("import sys; sys.modules['torch'] = None\n"
            "import sparta_amd.optim as o, sparta_amd as sa\n"
            "opt = sa.VbsSGD([], lr=0.5, momentum=0.9)\n"
            "opt.zero_grad()\n"
            "assert o.VbsSGD is sa.VbsSGD and sys.modules.get('torch') is None\n"
            "print('ok')\n")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.stdout, r.stderr)
    src = open(os.path.join(ROOT, "sparta_amd", "optim.py")).read()
    assert not [ln for ln in src.splitlines() if ln.startswith(("import torch", "from torch"))]
