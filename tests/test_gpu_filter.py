"""The fused spectral band-pass (gpu_spectral_filter_batch, wsp_plan_create_filter): forward FFT, real mask over
the packed elements, inverse -- or last sample and peak -- in one launch (L/WaveSpecZZ_1.0.4-core.mq5:561-578).

Reference, composed from the oracle (nothing of it is changed):
    P    = oracle.batch_spectrum(..., output="packed")
    ref  = oracle.fft_real_inverse(P[w] * mask)
    scale_w = max|mask| * max|oracle.fft_real_inverse(P[w])|     (the pre-FFT samples, not what the mask lets through)
Bars:
    series  max|x_f - ref|                   <= 1e-11 * scale_w
    last    |last - ref[N-1]|                <= 1e-11 * scale_w
    peak    |peak - max_(i>=1) |P * mask||   <= 1e-11 * max|P * mask|
The oracle's own pipeline differs from numpy.fft on these inputs by at most 3.8e-14 scale (N <= 4096) and
2.5e-13 scale (N = 16384), the closed-form last sample from ref[N-1] by at most 1.7e-13 scale: 1e-11 leaves
40 x over the checker's own error while any index, twiddle or scaling mistake is orders above it.
"""
import functools

import numpy as np
import pytest

import oracle
from wavespec_amd import bridge, spectral, synth

pytestmark = pytest.mark.gpu

BAR = 1e-11
W = 37
DW = [("none", "none", 0), ("mean", "none", 0), ("mean", "hann", 0), ("iir", "hann", 1024), ("mean", "bartlett", 0)]
MASKS = ["null", "band", "gauss", "random"]


def make_mask(name, n):
    if name == "null":
        return None
    if name == "band":
        return spectral.band_mask(n, 0.02, 0.30)
    if name == "gauss":
        return spectral.gaussian_mask(n, 32, 0.04, 1.0)
    return np.random.default_rng(n).uniform(-2.0, 2.0, n)  # independent values for Re and Im of every bin


@functools.lru_cache(maxsize=None)
def series_of(n, hop, nwin, seed=0):
    s = synth.random_walk((nwin - 1) * hop + n, seed=n + seed)
    s.setflags(write=False)
    return s


def reference(s, n, hop, detrend, window, period, mask, kalman=None):
    """(ref rows, scale per window, peak per window, max|P * mask| per window)."""
    P = oracle.batch_spectrum(s, n, hop, detrend, window, period, kalman=kalman, output="packed")
    m = np.ones(n) if mask is None else mask
    Y = P * m
    ref = np.stack([oracle.fft_real_inverse(y) for y in Y])
    pre = np.stack([oracle.fft_real_inverse(p) for p in P])
    scale = np.max(np.abs(m)) * np.max(np.abs(pre), axis=1)
    return ref, scale, np.max(np.abs(Y[:, 1:]), axis=1), np.max(np.abs(Y), axis=1)


@functools.lru_cache(maxsize=None)
def cached_reference(n, hop, nwin, detrend, window, period, mask_name):
    return reference(series_of(n, hop, nwin), n, hop, detrend, window, period, make_mask(mask_name, n))


def check_series(got, ref, scale, tag, rows=None):
    rows = np.arange(len(ref)) if rows is None else rows
    assert got.shape == ref.shape
    err = np.max(np.abs(got[rows] - ref[rows]), axis=1) / scale[rows]
    print(f"{tag} series: worst {np.max(err):.3e} of scale")
    assert np.all(err <= BAR), float(np.max(err))


def check_last(got, ref, scale, peak, ymax, tag, rows=None):
    rows = np.arange(len(ref)) if rows is None else rows
    assert got.shape == (len(ref), 2)
    e_last = np.abs(got[rows, 0] - ref[rows, -1]) / scale[rows]
    bound = np.where(ymax[rows] > 0, ymax[rows], 1.0)
    e_peak = np.abs(got[rows, 1] - peak[rows]) / bound
    print(f"{tag} last: sample {np.max(e_last):.3e} of scale, peak {np.max(e_peak):.3e} of max|Y|")
    assert np.all(e_last <= BAR), float(np.max(e_last))
    assert np.all(e_peak <= BAR), float(np.max(e_peak))


# ------------------------------------------------------------------ 1. parity matrix
@pytest.mark.parametrize("detrend,window,period", DW)
@pytest.mark.parametrize("n", [32, 64, 256, 1024, 2048, 4096, 16384])
def test_filter_parity(gpu_session, n, detrend, window, period):
    """N = 32 .. 16384: one thread per window; part of a wave; 8 and 32 threads; exactly one wave; two waves;
    eight waves with the 136 KiB slot.  37 windows at hop = N/2 + 3 (ragged last workgroup, odd overlapping
    hop), every mask, both modes."""
    hop = n // 2 + 3
    s = series_of(n, hop, W)
    for name in MASKS:
        mask = make_mask(name, n)
        ref, scale, peak, ymax = cached_reference(n, hop, W, detrend, window, period, name)
        tag = f"N={n} {detrend}/{window} {name}"
        check_series(bridge.spectral_filter_batch(s, n, hop, detrend, window, period, mask, "series"), ref, scale, tag)
        check_last(bridge.spectral_filter_batch(s, n, hop, detrend, window, period, mask, "last"), ref, scale, peak,
                   ymax, tag)


def test_filter_kalman(gpu_session):
    """The Kalman trend goes through the pre-pass into the workspace, then the fused kernel without a detrend."""
    n, hop = 1024, 515
    bridge.set_kalman_params(oracle.KALMAN_DEFAULTS)
    s = series_of(n, hop, W)
    mask = make_mask("band", n)
    ref, scale, peak, ymax = reference(s, n, hop, "kalman", "hann", 0, mask, kalman=oracle.KALMAN_DEFAULTS)
    check_series(bridge.spectral_filter_batch(s, n, hop, "kalman", "hann", 0, mask, "series"), ref, scale, "kalman")
    check_last(bridge.spectral_filter_batch(s, n, hop, "kalman", "hann", 0, mask, "last"), ref, scale, peak, ymax,
               "kalman")


# ------------------------------------------------------------------ 2. known answers, no oracle
@pytest.mark.parametrize("n", [32, 1024, 4096, 16384])
def test_null_mask_returns_the_window_without_nyquist(gpu_session, n):
    """No mask, detrend or window: x_f = x minus its Nyquist component (the packed layout has no slot for
    X_(N/2)), within the bar of test_gpu_parity.test_inverse_round_trip_single."""
    x = synth.random_walk(3 * n, seed=n).reshape(3, n)
    sign = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    want = x - (x @ sign / n)[:, None] * sign
    got = bridge.spectral_filter_batch(x.reshape(-1), n, n, "none", "none", 0, None, "series")
    err = np.max(np.abs(got - want)) / np.max(np.abs(x))
    print(f"N={n}: null-mask round trip {err:.3e} of max|x|")
    assert err <= 1e-13, err


@pytest.mark.parametrize("n", [32, 1024, 4096])
def test_one_hot_masks(gpu_session, n):
    """One packed element let through: x_f[j] = (2/N) Re X_k cos(2 pi k j/N) for element 2k, -(2/N) Im X_k
    sin(2 pi k j/N) for element 2k + 1, (1/N) X_0 for element 0, zero for element 1 (Im X_0 is ignored).  k = 0,
    1, B/2, M/2, M - 1 with M = N/2, B = N/16: thread 0's permuted slots, the self-paired bins and an ordinary
    thread.  X from numpy.fft.rfft; bar 1e-11 max|x| (scale_w of the module docstring with max|mask| = 1)."""
    m2, b = n // 2, n // 16
    x = synth.random_walk(n, seed=3 * n)
    X = np.fft.rfft(x)
    j = np.arange(n)
    scale = np.max(np.abs(x))
    for k in sorted({0, 1, b // 2, m2 // 2, m2 - 1}):
        for part in (0, 1):
            i = 2 * k + part
            mask = np.zeros(n)
            mask[i] = 1.0
            if k == 0:
                want = np.full(n, X[0].real / n) if part == 0 else np.zeros(n)
            elif part == 0:
                want = (2.0 / n) * X[k].real * np.cos(2 * np.pi * k * j / n)
            else:
                want = -(2.0 / n) * X[k].imag * np.sin(2 * np.pi * k * j / n)
            got = bridge.spectral_filter_batch(x, n, n, "none", "none", 0, mask, "series")[0]
            err = np.max(np.abs(got - want)) / scale
            last = bridge.spectral_filter_batch(x, n, n, "none", "none", 0, mask, "last")[0]
            comp = abs(X[k].real if part == 0 else X[k].imag)
            peak = 0.0 if i == 0 else (0.0 if i == 1 else comp)
            print(f"N={n} element {i}: series {err:.3e}, last {abs(last[0] - want[-1]) / scale:.3e} of max|x|")
            assert err <= BAR, (i, err)
            assert abs(last[0] - want[-1]) <= BAR * scale, i
            assert abs(last[1] - peak) <= BAR * max(comp, abs(X[0].real)), i


# ------------------------------------------------------------------ 3. device plans
def _wpb(n):
    tpw = n // 32  # M/16 threads per window; single-wave workgroups when a window fits one wave, else >= 128 threads
    return (64 if tpw <= 64 else max(tpw, 128)) // tpw


def _run_plan(torch, s, n, hop, nwin, detrend, window, period, mask, mode, grid=None):
    dev = torch.device("cuda", 0)
    plan = bridge.Plan.filter(0, n, hop, nwin, detrend, window, period, mode)
    plan.set_mask(mask)
    if grid is not None:
        plan.set_grid(grid)
    d_s = torch.from_numpy(np.array(s)).to(dev)
    d_o = torch.full((nwin * plan.record,), float("nan"), dtype=torch.float64, device=dev)
    plan.execute(d_s.data_ptr(), d_o.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    nbytes = plan.algorithmic_bytes
    plan.close()
    return d_o.view(nwin, -1).cpu().numpy(), nbytes


@pytest.mark.parametrize("n", [256, 4096])
def test_slot_reuse_across_grid_stride_iterations(gpu_session, n):
    """The window's LDS slot is used twice per window in the series form (forward exchanges, then conj Z and the
    inverse exchanges): one and two workgroups walking 3 WPB + 1 windows must give the default grid's result
    bit for bit."""
    torch = pytest.importorskip("torch")
    nwin, hop = 3 * _wpb(n) + 1, n // 2 + 3
    s = series_of(n, hop, nwin, seed=1)
    mask = make_mask("random", n)
    ref, scale, peak, ymax = reference(s, n, hop, "mean", "hann", 0, mask)
    for mode in ("series", "last"):
        base, _ = _run_plan(torch, s, n, hop, nwin, "mean", "hann", 0, mask, mode)
        if mode == "series":
            check_series(base, ref, scale, f"N={n} default grid")
        else:
            check_last(base, ref, scale, peak, ymax, f"N={n} default grid")
        for grid in (1, 2):
            got, _ = _run_plan(torch, s, n, hop, nwin, "mean", "hann", 0, mask, mode, grid)
            assert np.array_equal(got, base), (mode, grid)


@pytest.mark.parametrize("n,nwin", [(256, 20), (4096, 6)])
def test_filter_window_isolation(gpu_session, n, nwin):
    """hop = N; one window scaled by 1e6 and one holding a NaN sample, among windows that share their wave
    (N = 256: 8 windows per wave) or workgroup sequence: every other window meets its own bar in both modes --
    the last mode's shuffle reduction must not mix windows -- and the NaN window's record is NaN."""
    big, bad = 3, 5
    s = series_of(n, n, nwin, seed=2).copy()
    s[big * n:(big + 1) * n] *= 1e6
    s[bad * n + n // 3] = np.nan
    mask = make_mask("random", n)
    ref, scale, peak, ymax = reference(s, n, n, "mean", "none", 0, mask)
    rows = np.array([w for w in range(nwin) if w != bad])
    assert np.isfinite(ref[rows]).all()
    got = bridge.spectral_filter_batch(s, n, n, "mean", "none", 0, mask, "series")
    check_series(got, ref, scale, f"N={n} isolation", rows)
    assert np.isnan(got[bad]).all()
    got = bridge.spectral_filter_batch(s, n, n, "mean", "none", 0, mask, "last")
    check_last(got, ref, scale, peak, ymax, f"N={n} isolation", rows)
    assert np.isnan(got[bad]).all()


@pytest.mark.parametrize("n", [64, 1024, 8192])
def test_last_matches_series_and_plan_matches_host(gpu_session, n):
    """MTB_FILTER_LAST against element N - 1 of MTB_FILTER_SERIES on the same input (1e-12 of scale_w: both come
    from the same registers, only the closed-form sum differs from the transform), the plan's byte accounting,
    and the plan path against the host call (the same kernel: identical records)."""
    torch = pytest.importorskip("torch")
    hop = n // 2 + 3
    s = series_of(n, hop, W)
    mask = make_mask("gauss", n)
    _, scale, _, _ = cached_reference(n, hop, W, "mean", "hann", 0, "gauss")
    ser = bridge.spectral_filter_batch(s, n, hop, "mean", "hann", 0, mask, "series")
    last = bridge.spectral_filter_batch(s, n, hop, "mean", "hann", 0, mask, "last")
    err = np.max(np.abs(last[:, 0] - ser[:, -1]) / scale)
    print(f"N={n}: last against series[N-1] {err:.3e} of scale")
    assert err <= 1e-12, err
    p_ser, b_ser = _run_plan(torch, s, n, hop, W, "mean", "hann", 0, mask, "series")
    p_last, b_last = _run_plan(torch, s, n, hop, W, "mean", "hann", 0, mask, "last")
    assert np.array_equal(p_ser, ser) and np.array_equal(p_last, last)
    unique = (W - 1) * hop + n  # overlapping windows: every sample once; the mask is not counted
    assert b_ser == 8 * (unique + W * n) and b_last == 8 * (unique + W * 2)


def test_plan_mask_and_setters(gpu_session):
    """A filter plan starts with the all-ones mask, wsp_plan_set_mask replaces it (None restores it), a wrong
    length is refused, and the tuning setters other than the grid do not apply."""
    torch = pytest.importorskip("torch")
    n, hop, nwin = 256, 131, 9
    s = series_of(n, hop, nwin)
    dev = torch.device("cuda", 0)
    d_s = torch.from_numpy(np.array(s)).to(dev)
    d_o = torch.empty(nwin * n, dtype=torch.float64, device=dev)
    plan = bridge.Plan.filter(0, n, hop, nwin, "mean", "none", 0, "series")

    def run():
        plan.execute(d_s.data_ptr(), d_o.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return d_o.view(nwin, n).cpu().numpy()

    ones = run()
    assert np.array_equal(ones, bridge.spectral_filter_batch(s, n, hop, "mean", "none", 0, None, "series"))
    mask = make_mask("band", n)
    plan.set_mask(mask)
    assert np.array_equal(run(), bridge.spectral_filter_batch(s, n, hop, "mean", "none", 0, mask, "series"))
    plan.set_mask(None)
    assert np.array_equal(run(), ones)
    L = bridge.lib()
    assert L.wsp_plan_set_mask(plan.handle, bridge._dptr(mask), n - 1) == bridge.BAD_ARGS
    assert L.wsp_plan_set_variant(plan.handle, 1) == bridge.BAD_ARGS
    assert L.wsp_plan_set_algorithm(plan.handle, 1) == bridge.BAD_ARGS
    assert L.wsp_plan_set_topk(plan.handle, 8, 18.0, 200.0) == bridge.BAD_ARGS
    assert L.wsp_plan_set_chunk(plan.handle, 4) == bridge.BAD_ARGS
    plan.close()
    spec = bridge.Plan(0, n, hop, nwin, "mean", "hann")
    assert L.wsp_plan_set_mask(spec.handle, bridge._dptr(mask), n) == bridge.BAD_ARGS  # not a filter plan
    spec.close()


# ------------------------------------------------------------------ 4. the core indicator's loop
def test_core_wave(gpu_session):
    """spectral.core_wave over a 3000-bar random walk, N = 1024, against the reference's own sequence per bar:
    remove the mean, gpu_fft_real_forward, multiply by the mask, peak, gpu_fft_real_inverse, last sample."""
    n = 1024
    close = synth.random_walk(3000, seed=11)
    mask = spectral.band_mask(n, 0.02, 0.30)
    wave, power = spectral.core_wave(close, n, mask, "mean")
    bars = close.size - n + 1
    assert wave.shape == power.shape == (bars,)
    e_wave = e_pow = 0.0
    for j in range(bars):
        x = close[j:j + n] - np.mean(close[j:j + n])
        y = bridge.fft_real_forward(x) * mask
        back = bridge.fft_real_inverse(y)
        e_wave = max(e_wave, abs(wave[j] - back[-1]) / np.max(np.abs(x)))
        e_pow = max(e_pow, abs(power[j] - np.max(np.abs(y[1:]))) / np.max(np.abs(y)))
    print(f"core_wave: wave {e_wave:.3e} of scale, power {e_pow:.3e} of max|Y|")
    assert e_wave <= BAR and e_pow <= BAR
