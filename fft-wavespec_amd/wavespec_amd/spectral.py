"""Masks and the per-bar pipeline of the "core" indicator over the fused spectral filter.

The reference's ``Legacy/WaveSpecZZ_1.0.4-core.mq5`` runs, per bar: copy the last N closes, remove DC,
``gpu_fft_real_forward``, multiply the packed spectrum by a real mask, take the peak magnitude,
``gpu_fft_real_inverse``, and plots the last filtered sample and the peak.  ``bridge.spectral_filter_batch``
does all of it for every bar in one launch; this module builds the masks the indicator builds on the MQL side
and lines the records up with bars.

A mask has one real value per packed *element* (``P[2k] = Re X_k``, ``P[2k+1] = Im X_k``), exactly as the
reference applies it (``core.mq5:394-401``): it is not a per-bin gain.
"""
from __future__ import annotations

import numpy as np

from . import bridge


def band_mask(n: int, low: float, high: float) -> np.ndarray:
    """The pass band of ``BuildMaskArray`` (``core.mq5:227-239``): element i has ratio i/(n-1); 1 where
    low <= ratio <= high, else 0.  ``low`` and ``high`` are clamped to [0, 1] and ``high`` raised to ``low``
    as there.  The ZigZag blend (``:241-264``) is not applied."""
    low = max(0.0, min(1.0, float(low)))
    high = max(0.0, min(1.0, float(high)))
    if high < low:
        high = low
    ratio = np.zeros(n) if n <= 1 else np.arange(n, dtype=np.float64) / float(n - 1)
    return np.where((ratio < low) | (ratio > high), 0.0, 1.0)


def gaussian_mask(n: int, period: float, bandwidth: float, gain: float) -> np.ndarray:
    """The values of ``BuildConvolutionKernel`` (``core.mq5:271-281``): gain * exp(-(i/n - 1/period)^2 /
    (2 bandwidth^2)) with period >= 4, bandwidth in [1e-4, 0.5] and gain >= 0 clamped as there.  Offered as a
    mask only: what the DLL's "convolution" stage does with these values is not in the reference's source."""
    period = max(4.0, float(max(1, period)))
    bandwidth = max(0.0001, min(0.5, float(bandwidth)))
    gain = max(0.0, float(gain))
    sigma = 2.0 * bandwidth * bandwidth
    delta = np.arange(n, dtype=np.float64) / float(n) - 1.0 / period
    return gain * np.exp(-delta * delta / sigma)


def core_wave(close: np.ndarray, n: int, mask: np.ndarray | None, detrend: str = "mean"):
    """The core indicator's ``OnCalculate`` loop (``core.mq5:561-578``) as one ``MTB_FILTER_LAST`` batch at
    hop = 1 over a chronological ``close``.  Returns ``(wave, power)``, each of length ``len(close) - n + 1``:
    element j belongs to bar ``n - 1 + j`` (the window ending at that bar), ``wave`` = the last sample of the
    filtered window (``WaveBuffer``), ``power`` = max |Y[i]| over packed elements i >= 1 (``PowerBuffer``).

    ``core.mq5:565`` starts at bar ``n`` -- its window at offset 0 is skipped; this starts at bar ``n - 1``, the
    library's batch convention (window w covers ``close[w : w + n]``).  The DLL's DC-removal stage
    (``gpu_remove_dc_time_series`` with ``InpDcMode``) has no source in the reference: mapping it to the mean
    detrend is this build's choice (``detrend`` also takes "none" and "kalman"; the IIR trend needs a period and
    goes through ``bridge.spectral_filter_batch`` directly)."""
    rec = bridge.spectral_filter_batch(close, n, 1, detrend, "none", 0, mask, "last")
    return rec[:, 0].copy(), rec[:, 1].copy()
