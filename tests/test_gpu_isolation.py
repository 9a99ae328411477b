"""Window isolation: a window's record depends on that window's own N samples only.

The reference runs one FFT per window (L/WaveSpecZZ_1.0.2.mq5:884-974), so a bad tick or a missing bar
(NaN, Inf, MQL5's EMPTY_VALUE = DBL_MAX) spoils exactly the windows that contain it.  Several kernels here
carry state from window to window -- the hop = 1 sliding DFT (trackers slid across a segment, the mean path's
level), the top-k probe thresholds, the Kalman pre-pass tiles, the large-N workspace -- and every other parity
test feeds them one well-behaved data family.  Here one sample of a synth.random_walk series is contaminated
at index c and the windows are split by arithmetic alone:

    contaminated:  w * hop <= c < w * hop + N          clean: every other window

Requirements (include/mtbridge.h, wsp_plan_set_algorithm):
  * NaN / +Inf / DBL_MAX: the clean windows meet the usual bars (1e-10 fp64, 1e-5 fp32, full
    row and in band; _topk_bars for records) against the oracle run on the same contaminated series;
  * NaN / +Inf: every contaminated power row holds at least one non-finite value (DBL_MAX: no requirement --
    0 * DBL_MAX at a zero window weight is legitimately finite; contaminated top-k records: no requirement);
  * +100 added to the sample (~100 x the price level): every window of the batch at the usual bars;
  * per-window FFT kernels: the clean rows are bit-identical to the run with the sample restored.

Every sliding-DFT case also asserts that some clean windows FOLLOW the contaminant inside the segment that
slid across it (or, where the contaminant is the series' last sample, precede it there): those windows are
the point of the test.
"""
import numpy as np
import pytest

import oracle
from test_gpu_slide import _run, _topk_bars
from wavespec_amd import bridge, synth

pytestmark = pytest.mark.gpu

TOL = {"f64": 1e-10, "f32": 1e-5}
KALMAN = oracle.KALMAN_DEFAULTS
KINDS = ["nan", "inf", "dblmax", "p100"]
POLICY_SEG = 32  # the launchers' segment for a batch far below one round of resident workgroups


def contaminate(series, c, kind):
    s = series.copy()
    if kind == "p100":
        s[c] += 100.0
    else:
        s[c] = {"nan": np.nan, "inf": np.inf, "dblmax": np.finfo(float).max}[kind]
    return s


def sets(nwin, hop, n, c, min_clean=None):
    """(clean, dirty) window masks from c, hop and N alone; the clean set is at least half the batch unless
    the case states the count its shape gives (min_clean)."""
    w = np.arange(nwin)
    dirty = (w * hop <= c) & (c < w * hop + n)
    clean = ~dirty
    assert dirty.any()
    assert int(clean.sum()) >= ((nwin + 1) // 2 if min_clean is None else min_clean), int(clean.sum())
    return clean, dirty


def assert_neighbours(clean, c, seg, n):
    """hop = 1: clean windows after c has left, inside a segment [w0, w0 + seg) that read sample c (its samples
    are w0 .. w0 + seg + n - 2) -- or, when c is the series' last sample and nothing follows, before it entered."""
    w = np.arange(clean.size)
    w0 = (w // seg) * seg
    read_c = (w0 <= c) & (c <= w0 + seg + n - 2)
    after = clean & read_c & (w > c)
    before = clean & read_c & (w + n <= c)
    if c + 1 < clean.size:
        assert after.any()
    else:
        assert before.any()
    return after | before


def f32_round(s):
    with np.errstate(over="ignore"):
        return s.astype(np.float32).astype(np.float64)


def check_power(got, want, clean, dirty, n, tol, kind, tag=""):
    """The requirements above on power rows; prints each figure before it asserts."""
    if kind == "p100":
        clean = np.ones_like(clean)
    assert got.shape == want.shape
    assert np.isfinite(want[clean]).all()  # the oracle's clean rows
    g, r = got[clean], want[clean]
    nonfinite = int((~np.isfinite(g).all(axis=1)).sum())
    print(f"{tag} {kind}: {nonfinite} of {len(g)} clean windows non-finite")
    assert nonfinite == 0, nonfinite
    full = oracle.rel_err(g, r)
    inb = oracle.inband_err(g, r, *oracle.band(n))
    print(f"{tag} {kind}: full row {full:.3e}, in band {inb:.3e}")
    assert full <= tol, full
    assert inb <= tol, inb
    if kind in ("nan", "inf"):
        assert (~np.isfinite(got[dirty])).any(axis=1).all()  # a caller can see the window is unusable


# ------------------------------------------------------------------ 1. sliding DFT, power rows
SLIDE_SHAPES = [(512, 100, 300), (512, 100, 293), (512, 100, 1210), (512, 600, 50), (512, 0, 384)]
DW = [("none", "hann"), ("mean", "hann"), ("mean", "blackman"), ("none", "none")]
SLIDE_CASES = [(n, seg, c, d, w, "f64") for (n, seg, c) in SLIDE_SHAPES for (d, w) in DW]
SLIDE_CASES += [(n, seg, c, "mean", "hann", "f32") for (n, seg, c) in SLIDE_SHAPES if seg == 100]
SLIDE_CASES += [(1024, 100, 300, "mean", "hann", "f64")]  # the two-bins-per-thread sibling of N = 512


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,seg,c,detrend,window,prec", SLIDE_CASES)
def test_slide_power_isolation(gpu_session, n, seg, c, detrend, window, prec, kind):
    """hop = 1 power rows by the sliding DFT, 700 windows: the contaminant on a segment's first sample (100-window
    segments, c = 300), leaving mid-segment (293), entering only the last window (1210, the series' last sample),
    leaving inside a 600-window segment that spans two staging chunks (50), on a multiple of 128 under the
    policy's 32-window segments (384: 385 of the 700 windows contain it, so the clean set is the 315 that
    remain -- the only case below half the batch)."""
    torch = pytest.importorskip("torch")
    nwin = 700
    s = contaminate(synth.random_walk(nwin + n - 1, seed=n + c), c, kind)
    if prec == "f32":
        s = f32_round(s)
    clean, dirty = sets(nwin, 1, n, c, min_clean=315 if c == 384 else None)
    assert_neighbours(clean, c, seg or POLICY_SEG, n)
    plan = bridge.Plan(0, n, 1, nwin, detrend, window, 0, prec)
    plan.set_algorithm("slide")
    assert plan.algorithm() == "slide"
    if seg:
        plan.set_slide_segment(seg)
    got = _run(plan, s, torch, torch.float32 if prec == "f32" else torch.float64)
    plan.close()
    want = oracle.batch_spectrum(s, n, 1, detrend, window)
    check_power(got, want, clean, dirty, n, TOL[prec], kind, f"slide N={n} seg={seg} c={c} {detrend}/{window} {prec}")


# ------------------------------------------------------------------ 2. sliding DFT, top-k records
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("detrend", ["none", "mean"])
@pytest.mark.parametrize("c", [300, 549])
def test_slide_topk_isolation(gpu_session, c, detrend, kind):
    """hop = 1 top-8 records, N = 1024, 100-window segments: the probe-threshold scan (thresholds from the window
    16 earlier), the one-wave scan, the transposed scan and the chained seeds (variants 0, 1, 2, 6).  On the clean
    windows the three scans stay identical to each other, as on clean data, and all meet the oracle's bars.
    c = 549 leaves 150 clean windows of the 700 (550..699): the contaminant leaves mid-segment there."""
    torch = pytest.importorskip("torch")
    n, nwin, k, seg = 1024, 700, 8, 100
    s = contaminate(synth.random_walk(nwin + n - 1, seed=n + c), c, kind)
    clean, dirty = sets(nwin, 1, n, c, min_clean=150 if c == 549 else None)
    assert_neighbours(clean, c, seg, n)
    if kind == "p100":
        clean = np.ones_like(clean)
    outs = {}
    for v in (0, 1, 2, 6):
        plan = bridge.Plan(0, n, 1, nwin, detrend, "hann", output="topk")
        plan.set_topk(k, 18.0, 200.0)
        plan.set_algorithm("slide")
        plan.set_variant(v)
        plan.set_slide_segment(seg)
        assert plan.algorithm() == "slide"
        outs[v] = _run(plan, s, torch).reshape(nwin, k, 4)
        plan.close()
    want = oracle.batch_topk(s, n, 1, detrend, "hann", 0, None, k, 18.0, 200.0)
    spec = oracle.batch_spectrum(s, n, 1, detrend, "hann")
    kmin, kmax = oracle.band(n)
    assert np.isfinite(want[clean]).all() and np.isfinite(spec[clean]).all()
    for v, got in outs.items():
        bad = int((~np.isfinite(got[clean]).all(axis=(1, 2))).sum())
        print(f"topk c={c} {detrend} {kind} variant {v}: {bad} of {int(clean.sum())} clean records non-finite")
    for v, got in outs.items():
        assert np.isfinite(got[clean]).all(), v
        _topk_bars(got[clean], want[clean], spec[clean][:, kmin:kmax + 1].max(axis=1), max_swaps=4)
    for v in (1, 2):
        assert np.array_equal(outs[0][clean], outs[v][clean]), v


# ------------------------------------------------------------------ 3. grouped plans
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("where", ["first", "last"])
@pytest.mark.parametrize("mode", ["auto", "per-length"])
def test_group_isolation(gpu_session, mode, where, kind):
    """Grouped hop = 1 plan, members of 512 / 1024 / 512 samples with 700 / 300 / 40 windows, mean detrend (the
    members' levels) and 100-window segments: a contaminant in the first member (c = 300, a segment's first
    sample) or in the last (c = 10) through the mixed-length persistent launch and the per-length launches.
    Every clean window of every member against the oracle; the second member is untouched."""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda", 0)
    lens, nwins, seg = [512, 1024, 512], [700, 300, 40], 100
    hs = [synth.random_walk(nw + n - 1, seed=400 + i) for i, (n, nw) in enumerate(zip(lens, nwins))]
    m, c = (0, 300) if where == "first" else (2, 10)
    hs[m] = contaminate(hs[m], c, kind)
    clean, dirty = sets(nwins[m], 1, lens[m], c)
    assert_neighbours(clean, c, seg, lens[m])
    series = [torch.from_numpy(h).to(dev) for h in hs]
    outs = [torch.empty(nw * (n // 2), dtype=torch.float64, device=dev) for n, nw in zip(lens, nwins)]
    g = bridge.Group(0, lens, nwins, "mean", "hann")
    g.set_mode(mode)
    g.set_segment(seg)
    assert g.launches == (1 if mode == "auto" else 2)
    g.execute([x.data_ptr() for x in series], [o.data_ptr() for o in outs], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    g.close()
    for i, (n, nw) in enumerate(zip(lens, nwins)):
        got = outs[i].cpu().numpy().reshape(nw, n // 2)
        want = oracle.batch_spectrum(hs[i], n, 1, "mean", "hann")
        if i == m:
            check_power(got, want, clean, dirty, n, TOL["f64"], kind, f"group {mode} member {i}")
        else:
            every = np.ones(nw, bool)
            check_power(got, want, every, ~every, n, TOL["f64"], "clean", f"group {mode} member {i}")


# ------------------------------------------------------------------ 4. host batch path
def test_host_batch_isolation(gpu_session):
    """gpu_spectrum_batch / gpu_spectrum_topk_batch at hop = 1 (the indicator's batch warm-up): AUTO takes the
    sliding DFT, NaN at c = 384 (the first sample of a policy segment; 315 clean windows of 700)."""
    nwin, c = 700, 384
    for n, topk in ((512, False), (1024, True)):
        s = contaminate(synth.random_walk(nwin + n - 1, seed=n + 1), c, "nan")
        clean, dirty = sets(nwin, 1, n, c, min_clean=315)
        assert_neighbours(clean, c, POLICY_SEG, n)
        plan = bridge.Plan(0, n, 1, nwin, "mean", "hann", output="topk" if topk else "power")
        assert plan.algorithm() == "slide"  # the policy has not silently changed under the test
        plan.close()
        spec = oracle.batch_spectrum(s, n, 1, "mean", "hann")
        if not topk:
            got = bridge.spectrum_batch(s, n, 1, "mean", "hann")
            check_power(got, spec, clean, dirty, n, TOL["f64"], "nan", f"host batch N={n}")
        else:
            got = bridge.spectrum_topk_batch(s, n, 1, "mean", "hann")
            want = oracle.batch_topk(s, n, 1, "mean", "hann", 0, None, 8, 18.0, 200.0)
            kmin, kmax = oracle.band(n)
            assert np.isfinite(want[clean]).all()
            bad = int((~np.isfinite(got[clean]).all(axis=(1, 2))).sum())
            print(f"host topk batch N={n}: {bad} of {int(clean.sum())} clean records non-finite")
            assert bad == 0, bad
            _topk_bars(got[clean], want[clean], spec[clean][:, kmin:kmax + 1].max(axis=1), max_swaps=4)


# ------------------------------------------------------------------ 5. per-window FFT kernels: bit identity
def _identity(run, series, c, clean, kinds=("nan", "inf", "p100")):
    base = run(series)
    for kind in kinds:
        got = run(contaminate(series, c, kind))
        assert got.shape == base.shape
        assert np.array_equal(got[clean], base[clean]), kind


@pytest.mark.parametrize("prec", ["f64", "f32"])
@pytest.mark.parametrize("hop_n", [True, False])
@pytest.mark.parametrize("n", [64, 1024, 4096])
@pytest.mark.parametrize("detrend,period", [("none", 0), ("mean", 0), ("iir", 37)])
def test_fft_power_bit_identity(gpu_session, detrend, period, n, hop_n, prec):
    """27 windows (N = 64: one workgroup holds them all), hop = N (the contaminant mid-batch, window 13) and
    hop = 7 (overlapping, unaligned windows; the contaminant in windows 0 and 1): the clean rows do not change
    by one bit when the contaminated sample is restored."""
    nwin, hop = 27, (n if hop_n else 7)
    s = synth.random_walk((nwin - 1) * hop + n, seed=n + hop)
    c = 13 * n + n // 3 if hop_n else 10
    clean, _ = sets(nwin, hop, n, c)
    _identity(lambda x: bridge.spectrum_batch(x, n, hop, detrend, "hann", period, prec), s, c, clean)


def test_fft_packed_bit_identity(gpu_session):
    n, nwin = 1024, 27
    s = synth.random_walk(nwin * n, seed=5)
    c = 13 * n + 7
    clean, _ = sets(nwin, n, n, c)
    _identity(lambda x: bridge.spectrum_batch(x, n, n, "none", "hann", output="packed"), s, c, clean)


@pytest.mark.parametrize("output", ["phase", "topk_phase"])
def test_fft_phase_bit_identity(gpu_session, output):
    """Phase rows and top-k phase records at N = 2048: the unwrap runs along the bins of one window and its
    state must not leak into the workgroup's next window."""
    n, nwin = 2048, 27
    s = synth.random_walk(nwin * n, seed=6)
    c = 13 * n + 1000
    clean, _ = sets(nwin, n, n, c)
    if output == "phase":
        run = lambda x: bridge.spectrum_batch(x, n, n, "none", "hann", output="phase")  # noqa: E731
    else:
        run = lambda x: bridge.spectrum_topk_phase_batch(x, n, n, "none", "hann")  # noqa: E731
    _identity(run, s, c, clean)


def test_fft_hop1_bit_identity(gpu_session):
    """hop = 1 through the per-window FFT kernel (wsp_plan_set_algorithm "fft"), N = 512, 300 windows."""
    torch = pytest.importorskip("torch")
    n, nwin, c = 512, 300, 700
    s = synth.random_walk(nwin + n - 1, seed=8)
    clean, _ = sets(nwin, 1, n, c)  # windows 189 .. 299 hold sample 700

    def run(x):
        plan = bridge.Plan(0, n, 1, nwin, "mean", "hann")
        plan.set_algorithm("fft")
        assert plan.algorithm() == "fft"
        out = _run(plan, x, torch)
        plan.close()
        return out

    _identity(run, s, c, clean)


@pytest.mark.parametrize("n", [64, 2048])
def test_inverse_bit_identity(gpu_session, n):
    """gpu_fft_real_inverse_batch, 37 packed spectra, NaN / Inf in one of them."""
    rows = 37
    spectra = np.stack([bridge.fft_real_forward(synth.sine_noise_window(n, seed=i)) for i in range(rows)])
    base = bridge.fft_real_inverse_batch(spectra)
    clean = np.arange(rows) != 17
    for v in (np.nan, np.inf):
        bad = spectra.copy()
        bad[17, n // 2 + 1] = v
        got = bridge.fft_real_inverse_batch(bad)
        assert np.array_equal(got[clean], base[clean])
        assert not np.isfinite(got[17]).all()


# ------------------------------------------------------------------ 6. Kalman pre-pass
@pytest.mark.parametrize("kind", ["nan", "inf"])
@pytest.mark.parametrize("pos", ["first", "cold", "mid"])
@pytest.mark.parametrize("hop_n", [True, False])
@pytest.mark.parametrize("n", [256, 1024])
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_kalman_isolation(gpu_session, prec, n, hop_n, pos, kind):
    """The Kalman trend pre-pass runs tiles of 64 windows (130 windows: two tiles and a ragged one), in fp32 as
    a sequential filter (N = 256) or two time segments verified at the hand-over (N >= 1024, the second starting
    cold at sample L0 - WU = (N + 256)/2 - 256), with a per-wave guard that sends a wave to another basis.  A
    non-finite sample on window 70's first sample, on its cold-start sample (N = 256 has none: its last sample)
    or mid-window must not change what the clean windows of its tile and wave compute."""
    nwin, hop = 130, (n if hop_n else 37)
    off = {"first": 0, "cold": (n + 256) // 2 - 256 if n >= 1024 else n - 1, "mid": n // 2 + 5}[pos]
    c = 70 * hop + off
    s = contaminate(synth.random_walk((nwin - 1) * hop + n, seed=n + hop), c, kind)
    if prec == "f32":
        s = f32_round(s)
    clean, dirty = sets(nwin, hop, n, c)
    assert clean[64:128].any() and dirty[64:128].any()  # clean and contaminated windows share the middle tile
    got = bridge.spectrum_batch(s, n, hop, "kalman", "hann", 0, prec)
    want = oracle.batch_spectrum(s, n, hop, "kalman", "hann", 0, kalman=KALMAN)
    check_power(got, want, clean, dirty, n, TOL[prec], kind, f"kalman N={n} hop={hop} {pos} {prec}")


# ------------------------------------------------------------------ 7. large N
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("detrend", ["mean", "none"])
def test_large_isolation(gpu_session, detrend, variant):
    """N = 32768 (the four-step transform and its workspace), 6 windows, NaN in window 2: the other five rows
    against the oracle."""
    torch = pytest.importorskip("torch")
    n, nwin = 32768, 6
    c = 2 * n + 12345
    s = contaminate(synth.random_walk(nwin * n, seed=32), c, "nan")
    clean, dirty = sets(nwin, n, n, c)
    plan = bridge.Plan(0, n, n, nwin, detrend, "hann")
    plan.set_variant(variant)
    got = _run(plan, s, torch)
    plan.close()
    want = oracle.batch_spectrum(s, n, n, detrend, "hann")
    assert np.isfinite(want[clean]).all()
    assert np.isfinite(got[clean]).all()
    err = oracle.rel_err(got[clean], want[clean])
    print(f"large {detrend} variant {variant}: full row {err:.3e}")
    assert err <= 1e-10, err
    assert (~np.isfinite(got[dirty])).any(axis=1).all()
