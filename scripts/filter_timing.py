#!/usr/bin/env python3
"""Times the fused spectral filter against the unfused pipeline and the north-star power plan, interleaved
in one process (bench.py's method: HIP events around K back-to-back launches after W untimed ones, inputs
resident in HBM, synth.random_walk_torch).

Shape: 65536 windows x 4096 samples, hop = N, fp64, mean detrend, no window, band_mask(0.02, 0.30).
  (a) fused_series    wsp_plan_create_filter, MTB_FILTER_SERIES
  (b) unfused         packed forward plan -> in-place torch multiply by the mask -> inverse plan
  (c) fused_last      wsp_plan_create_filter, MTB_FILTER_LAST
  (d) power           the north-star power plan (mean detrend, no window)
Each round times (a), (b), (c), (d) in turn; the reported time of a form is the median over rounds, its spread
(max - min) / median.  Algorithmic bytes: unique input samples + records (the unfused pipeline: the sum over
its three passes, the mask pass reading and writing the packed spectra); HBM fraction = bytes / time / 8 TB/s.

Usage: python scripts/filter_timing.py [--windows 65536] [--n 4096] [--steps 20] [--warmup 5] [--rounds 7]
       [--out profiles/filter/timing.json]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "fft-wavespec_amd"))

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E (bench.py)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=65536)
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "filter" / "timing.json"))
    args = ap.parse_args(argv)

    import torch

    from wavespec_amd import bridge, spectral, synth

    if not torch.cuda.is_available():
        print("filter_timing: no GPU visible (times are measured on the device only)", file=sys.stderr)
        return 2
    n, w = args.n, args.windows
    dev = torch.device("cuda", 0)
    bridge.lib()
    stream = torch.cuda.current_stream().cuda_stream
    series = synth.random_walk_torch(w * n, 1, dev, torch.float64)
    mask = spectral.band_mask(n, 0.02, 0.30)
    d_mask = torch.from_numpy(mask).to(dev)
    d_rows = torch.empty(w * n, dtype=torch.float64, device=dev)     # filtered windows / packed spectra
    d_back = torch.empty(w * n, dtype=torch.float64, device=dev)     # the unfused pipeline's samples
    d_last = torch.empty(w * 2, dtype=torch.float64, device=dev)
    d_pow = torch.empty(w * (n // 2), dtype=torch.float64, device=dev)
    spec_view = d_rows.view(w, n)

    fused = bridge.Plan.filter(0, n, n, w, "mean", "none", 0, "series")
    fused.set_mask(mask)
    last = bridge.Plan.filter(0, n, n, w, "mean", "none", 0, "last")
    last.set_mask(mask)
    fwd = bridge.Plan(0, n, n, w, "mean", "none", 0, "f64", "packed")
    inv = bridge.Plan.inverse(0, n, w)
    power = bridge.Plan(0, n, n, w, "mean", "none", 0, "f64", "power")

    def run_unfused():
        fwd.execute(series.data_ptr(), d_rows.data_ptr(), stream)
        spec_view.mul_(d_mask)
        inv.execute(d_rows.data_ptr(), d_back.data_ptr(), stream)

    forms = {
        "fused_series": (lambda: fused.execute(series.data_ptr(), d_rows.data_ptr(), stream), fused.algorithmic_bytes),
        "unfused": (run_unfused, fwd.algorithmic_bytes + 2 * 8 * w * n + inv.algorithmic_bytes),
        "fused_last": (lambda: last.execute(series.data_ptr(), d_last.data_ptr(), stream), last.algorithmic_bytes),
        "power": (lambda: power.execute(series.data_ptr(), d_pow.data_ptr(), stream), power.algorithmic_bytes),
    }

    # the fused and unfused pipelines compute the same samples (checked before anything is timed)
    forms["fused_series"][0]()
    torch.cuda.synchronize()
    got = d_rows.clone()
    run_unfused()
    torch.cuda.synchronize()
    diff = float((got - d_back).abs().max() / d_back.abs().max())
    print(f"fused against unfused samples: max difference {diff:.3e} of the largest sample", flush=True)

    def time_ms(step) -> float:
        for _ in range(args.warmup):
            step()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.steps):
            step()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / args.steps

    times = {k: [] for k in forms}
    for r in range(args.rounds):
        for k, (step, _) in forms.items():
            times[k].append(time_ms(step))
        print(f"round {r}: " + ", ".join(f"{k} {times[k][-1]:.4f} ms" for k in forms), flush=True)

    result = {"shape": {"windows": w, "n": n, "hop": n, "precision": "f64", "detrend": "mean", "window": "none",
                        "mask": "band_mask(0.02, 0.30)"},
              "method": {"steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
                         "timer": "HIP events around the timed launches, forms interleaved per round"},
              "device": torch.cuda.get_device_name(0), "fused_vs_unfused_max_rel_diff": diff, "forms": {}}
    for k, (_, nbytes) in forms.items():
        med = statistics.median(times[k])
        result["forms"][k] = {"ms_median": round(med, 4), "ms_min": round(min(times[k]), 4),
                              "ms_max": round(max(times[k]), 4),
                              "spread": round((max(times[k]) - min(times[k])) / med, 4),
                              "algorithmic_bytes": int(nbytes),
                              "hbm_fraction": round(nbytes / (med * 1e-3) / (HBM_PEAK_GBS * 1e9), 4)}
    f = result["forms"]
    result["fused_series_over_unfused"] = round(f["fused_series"]["ms_median"] / f["unfused"]["ms_median"], 4)
    result["fused_last_over_power"] = round(f["fused_last"]["ms_median"] / f["power"]["ms_median"], 4)
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))
    for p in (fused, last, fwd, inv, power):
        p.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
