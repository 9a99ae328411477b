"""CPU tests of the fused spectral filter's C ABI and of the mask builders (no GPU needed: every argument
check of gpu_spectral_filter_batch comes before the session lookup, as in test_abi.test_bad_modes_and_shapes)."""
import ctypes as C
import math

import numpy as np
import pytest

from conftest import GPU
from wavespec_amd import bridge, spectral


def _call(series, n, hop, detrend, window, period, mask, mask_len, mode, out, out_cap):
    got = C.c_int32(7)
    st = bridge.lib().gpu_spectral_filter_batch(
        bridge._dptr(series), series.size, n, hop, detrend, window, period, None if mask is None else bridge._dptr(mask),
        mask_len, mode, None if out is None else bridge._dptr(out), out_cap, C.byref(got))
    return st, got.value


def test_filter_bad_arguments():
    s = np.zeros(40000)
    out = np.zeros(40000)
    m = np.ones(1024)
    ok = dict(series=s, n=1024, hop=512, detrend=1, window=0, period=0, mask=m, mask_len=1024, mode=0, out=out,
              out_cap=out.size)
    bad = [dict(mode=2), dict(mode=-1),                       # bad mode
           dict(mask_len=1023), dict(mask_len=512), dict(mask=None, mask_len=1024), dict(mask_len=0),  # bad mask_len
           dict(n=32768, mask=np.ones(32768), mask_len=32768),  # above the single-workgroup transform
           dict(out=None),                                      # null out
           dict(out_cap=1023), dict(mode=1, out_cap=1),         # below one record
           dict(n=1000, mask=np.ones(1000), mask_len=1000), dict(hop=0), dict(detrend=9), dict(window=7)]
    for change in bad:
        st, got = _call(**{**ok, **change})
        assert st == bridge.BAD_ARGS and got == 0, change
    st, _ = _call(**{**ok, "n": 32768, "mask": np.ones(32768), "mask_len": 32768})
    assert st == bridge.BAD_ARGS and "16384" in bridge.last_error()


@pytest.mark.skipif(GPU, reason="checks the no-GPU behaviour")
def test_filter_without_session_is_backend_unavailable():
    s = np.zeros(4096)
    out = np.zeros(4096)
    for mask, mlen, mode in ((np.ones(1024), 1024, 0), (None, 0, 1)):
        st, got = _call(s, 1024, 1024, 1, 0, 0, mask, mlen, mode, out, out.size)
        assert st == bridge.BACKEND_UNAVAILABLE and got == 0
    assert bridge.lib().wsp_plan_create_filter(0, 1024, 1024, 4, 1, 0, 0, 0) == 0


def test_set_mask_needs_a_filter_plan():
    m = np.ones(1024)
    assert bridge.lib().wsp_plan_set_mask(987654321, bridge._dptr(m), 1024) == bridge.BAD_ARGS
    assert bridge.lib().wsp_plan_set_mask(987654321, None, 0) == bridge.BAD_ARGS


def test_band_mask_values():
    m = spectral.band_mask(11, 0.2, 0.5)  # ratio = i / 10; both edges belong to the band
    assert m.tolist() == [0, 0, 1, 1, 1, 1, 0, 0, 0, 0, 0]
    m = spectral.band_mask(1024, 0.02, 0.30)  # ratio = i / 1023: 20/1023 < 0.02 <= 21/1023, 306/1023 <= 0.30 < 307/1023
    assert m[20] == 0 and m[21] == 1 and m[306] == 1 and m[307] == 0 and m.sum() == 286
    assert spectral.band_mask(8, 0.6, 0.2).tolist() == [0] * 8  # high raised to low = 0.6: no i/7 equals it
    assert spectral.band_mask(5, -1.0, 2.0).tolist() == [1] * 5  # clamped to [0, 1]
    assert spectral.band_mask(1, 0.0, 1.0).tolist() == [1]


def test_gaussian_mask_values():
    m = spectral.gaussian_mask(8, 4, 0.5, 2.0)  # target 1/4, sigma = 2 * 0.25 = 0.5
    assert m[2] == 2.0
    assert m[0] == pytest.approx(2.0 * math.exp(-0.125), rel=1e-15)
    assert m[6] == pytest.approx(2.0 * math.exp(-0.5), rel=1e-15)
    # clamps: period >= 4, bandwidth in [1e-4, 0.5], gain >= 0
    assert np.array_equal(spectral.gaussian_mask(8, 2, 9.0, 2.0), m)
    assert spectral.gaussian_mask(8, 4, 0.5, -3.0).tolist() == [0] * 8
    m = spectral.gaussian_mask(1024, 32, 0.04, 1.0)
    assert m[32] == 1.0 and m[0] == pytest.approx(math.exp(-(1 / 32) ** 2 / 0.0032), rel=1e-14)
