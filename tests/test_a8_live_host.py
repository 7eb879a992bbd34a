"""The fp8 image with a live-block set without a GPU: the two entry points are in the built library, DeviceVBS has their methods, and BlockPruner refuses
a8_live=True without skip_pruned=True and together with live_forward=True."""
import pytest

import sparta_amd as sa
from sparta_amd import _lib


def test_symbols_resolve():
    for name in ("sparta_vbs_set_a8_live", "sparta_vbs_a8_live_info"):
        assert name in _lib.SYMBOLS, name
        assert hasattr(_lib.lib, name), name
    assert len(_lib.lib.sparta_vbs_set_a8_live.argtypes) == 3 and len(_lib.lib.sparta_vbs_a8_live_info.argtypes) == 3


def test_device_methods_exist():
    assert callable(getattr(sa.DeviceVBS, "set_a8_live")) and callable(getattr(sa.DeviceVBS, "a8_live_info"))
    for needle in ("set_a8_live",):
        assert needle in sa.DeviceVBS.set_forward_a8.__doc__ and needle in sa.DeviceVBS.set_live_forward.__doc__


def test_pruner_refusals():
    with pytest.raises(ValueError, match="skip_pruned"):
        sa.BlockPruner([], a8_live=True)
    with pytest.raises(ValueError, match="live_forward"):
        sa.BlockPruner([], skip_pruned=True, live_forward=True, a8_live=True)
    p = sa.BlockPruner([], skip_pruned=True, a8_live=True)
    assert p.a8_live and not p.live_forward
    assert not sa.BlockPruner([], skip_pruned=True).a8_live
