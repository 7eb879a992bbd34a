"""Live steps (sparta_vbs_set_live_steps) without a GPU: the entry is exported with the declared prototype and refuses a NULL handle; BlockPruner validates
live_steps; and live_step_ref, the numpy float32 restatement of the contract "WITH A LIVE-BLOCK SET INSTALLED AND LIVE STEPS ON" of include/sparta_amd.h,
which tests/test_live_step_gpu.py imports as its oracle: on inputs whose dead blocks are +0 it gives what the unmasked references give."""
import ctypes as C
import os

import numpy as np
import pytest

import sparta_amd as sa
from sparta_amd import _lib
from sparta_amd._lib import lib

import _live as L
from test_adam_step_host import adam_ref, fresh_state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32

SGD_CONFIGS = [dict(lr=0.5), dict(lr=0.25, momentum=0.9), dict(lr=0.5, momentum=0.9, weight_decay=0.01), dict(lr=0.25, weight_decay=0.01, grad_scale=0.5)]
ADAM_CONFIGS = [dict(lr=1e-2), dict(lr=1e-2, weight_decay=0.01), dict(lr=1e-2, weight_decay=0.01, decoupled=False, grad_scale=0.5)]


def sgd_ref(W, G, M, cfg):
    """sparta_vbs_sgd_step in numpy float32, one rounding per operation (the order include/sparta_amd.h pins).  Returns (W, M) after the step; M is
    returned as it came when momentum == 0."""
    lr, mom, wd, gs = (f32(cfg.get(k, d)) for k, d in (("lr", None), ("momentum", 0.0), ("weight_decay", 0.0), ("grad_scale", 1.0)))
    W, g, M = np.asarray(W, f32), np.asarray(G, f32), np.asarray(M, f32)
    if gs != 1:
        g = g * gs
    if wd != 0:
        g = g + wd * W
    if mom != 0:
        M = mom * M + g
        g = M
    out = W - lr * g
    assert out.dtype == f32 and M.dtype == f32
    return out, M


def live_step_ref(kind, W, G, M, V, S, cfg, live, coef=None, skip=False):
    """The contract of a live step.  kind: "sgd" or "adam"; W, G, M, V: float32 arrays in the mab layout (V and S unused by "sgd"); live: per element, True
    where its block is live (_live.element_keep); coef, skip: words 7 and 8 of a control record (coef=None: no record; the oracle takes grad_scale == 1
    with a record, so that g * coef is the one rounding the kernels do).
    Returns (W, M, V, S, image): live elements with the pinned arithmetic, dead elements of W, M, V as they came -- never read, so a NaN there stays and
    reaches nothing -- S as the plain step leaves it, and `image` = the values the step's own kernel hands to the images: the new W where live, +0.0 where dead."""
    W, G, M, V = (np.array(a, f32) for a in (W, G, M, V))
    live = np.asarray(live, bool)
    Wn, Mn, Vn, Sn = W.copy(), M.copy(), V.copy(), np.array(S).view(np.uint32).copy()
    if not skip:
        g = G[live]
        if coef is not None:
            assert cfg.get("grad_scale", 1.0) == 1.0
            g = g * f32(coef)
        if kind == "sgd":
            Wn[live], m = sgd_ref(W[live], g, M[live], cfg)
            if cfg.get("momentum", 0.0) != 0:
                Mn[live] = m
        else:
            Wn[live], Mn[live], Vn[live], Sn = adam_ref(W[live], g, M[live], V[live], S, cfg)
    image = np.where(live, Wn, f32(0.0)).astype(f32)
    return Wn, Mn, Vn, Sn, image


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def test_symbol_and_prototype():
    assert "sparta_vbs_set_live_steps" in _lib.SYMBOLS and hasattr(lib, "sparta_vbs_set_live_steps")
    fn = lib.sparta_vbs_set_live_steps
    assert list(fn.argtypes) == [C.c_void_p, C.c_int32, C.c_void_p]
    hdr = open(os.path.join(ROOT, "include", "sparta_amd.h")).read()
    assert "int sparta_vbs_set_live_steps(sparta_vbs_t* A, int32_t enable, void* stream);" in hdr
    assert "WITH A LIVE-BLOCK SET INSTALLED AND LIVE STEPS ON" in hdr


def test_null_handle_is_invalid():
    for enable in (0, 1):
        assert lib.sparta_vbs_set_live_steps(None, enable, None) == _lib.ERR_INVALID
        msg = lib.sparta_last_error().decode()
        assert "sparta_vbs_set_live_steps" in msg and "NULL" in msg, msg


def test_block_pruner_validates_live_steps():
    pytest.importorskip("torch")
    with pytest.raises(ValueError, match="skip_pruned"):
        sa.BlockPruner([], live_steps=True)
    with pytest.raises(ValueError, match="skip_pruned"):
        sa.BlockPruner([], skip_pruned=False, live_steps=True)
    p = sa.BlockPruner([], skip_pruned=True, live_steps=True)
    assert p.skip_pruned and p.live_steps
    assert not sa.BlockPruner([], skip_pruned=True).live_steps


def _operands(key, name, seed):
    T = L.table(key, None)
    live = L.element_keep(T, L.mask(key, None, name))
    n = len(live)
    rng = np.random.default_rng(seed)
    W, G, M, V = (rng.uniform(-1, 1, n).astype(f32) for _ in range(4))
    V = np.abs(V)
    return live, W, G, M, V


@pytest.mark.parametrize("name", ["all", "none", "second", "rand50"])
@pytest.mark.parametrize("key", ["small", "zrows", "w13z"])
def test_on_dead_zero_inputs_the_masked_references_equal_the_unmasked(key, name):
    live, W, G, M, V = _operands(key, name, 8100)
    for a in (W, G, M, V):
        a[~live] = 0.0
    for cfg in SGD_CONFIGS:
        w, m, _, _, image = live_step_ref("sgd", W, G, M, V, fresh_state(), cfg, live)
        w0, m0 = sgd_ref(W, G, M, cfg)
        assert np.array_equal(bits(w), bits(w0)) and np.array_equal(bits(image), bits(w0)), (key, name, cfg)
        assert np.array_equal(bits(m), bits(m0 if cfg.get("momentum", 0.0) != 0 else M)), (key, name, cfg)
        assert not bits(w)[~live].any()
    for cfg in ADAM_CONFIGS:
        S = fresh_state()
        Wa, Ma, Va = W, M, V
        Wb, Mb, Vb, Sb = W, M, V, S
        for _ in range(3):
            Wa, Ma, Va, S, image = live_step_ref("adam", Wa, G, Ma, Va, S, cfg, live)
            Wb, Mb, Vb, Sb = adam_ref(Wb, G, Mb, Vb, Sb, cfg)
            for x, y in ((Wa, Wb), (Ma, Mb), (Va, Vb), (image, Wb)):
                assert np.array_equal(bits(x), bits(y)), (key, name, cfg)
            assert np.array_equal(S, Sb)
        assert not bits(Wa)[~live].any() and not bits(Ma)[~live].any() and not bits(Va)[~live].any()


def test_dead_elements_are_not_looked_at():
    live, W, G, M, V = _operands("zrows", "second", 8200)
    assert (~live).any() and live.any()
    W[~live] = 0.0
    Gp, Mp, Vp = G.copy(), M.copy(), V.copy()
    poison = np.array([np.nan, np.inf, 1e30], f32)
    for a in (Gp, Mp, Vp):
        a[~live] = poison[np.arange(int((~live).sum())) % 3]
    for kind, cfg in (("sgd", SGD_CONFIGS[2]), ("adam", ADAM_CONFIGS[1])):
        clean = live_step_ref(kind, W, np.where(live, G, 0), np.where(live, M, 0), np.where(live, V, 0), fresh_state(), cfg, live)
        got = live_step_ref(kind, W, Gp, Mp, Vp, fresh_state(), cfg, live)
        for i in range(3):
            assert np.array_equal(bits(got[i])[live], bits(clean[i])[live])
        assert np.array_equal(bits(got[1])[~live], bits(Mp)[~live]) and np.array_equal(bits(got[2])[~live], bits(Vp)[~live])
        assert np.isfinite(got[4]).all() and np.array_equal(bits(got[4]), bits(clean[4])) and not bits(got[0])[~live].any()
        # a control record: coef multiplies g; skip leaves W, M, V, S alone and still hands +0.0 for the dead blocks to the image
        cfg1 = dict(cfg, grad_scale=1.0)
        half = live_step_ref(kind, W, Gp, Mp, Vp, fresh_state(), cfg1, live, coef=0.5)
        want = live_step_ref(kind, W, (Gp * f32(0.5)).astype(f32), Mp, Vp, fresh_state(), cfg1, live)
        assert all(np.array_equal(bits(a)[live], bits(b)[live]) for a, b in zip(half[:3], want[:3]))
        skipped = live_step_ref(kind, W, Gp, Mp, Vp, fresh_state(), cfg1, live, coef=0.5, skip=True)
        assert np.array_equal(bits(skipped[0]), bits(W)) and np.array_equal(bits(skipped[1]), bits(Mp)) and np.array_equal(skipped[3], fresh_state())
        assert np.array_equal(bits(skipped[4]), bits(W))
