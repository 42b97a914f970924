"""ycnr_als_step_implicit_wide without a GPU: the entry point is exported and bound, and a null handle is refused before any
device is touched."""
import ycnr_als
from ycnr_als import _lib


def test_symbol_is_bound_and_refuses_a_null_handle():
    L = _lib.load()
    assert "ycnr_als_step_implicit_wide" in _lib.EXPORTS and len(L.ycnr_als_step_implicit_wide.argtypes) == 5
    assert L.ycnr_version() == 4  # additions only
    assert callable(ycnr_als.AlsDevice.step_implicit_wide)
    assert L.ycnr_als_step_implicit_wide(None, 0, 0.5, None, None) == _lib.ERR_INVALID
