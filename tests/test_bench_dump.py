"""bench.py's plain / --full split and --dump-outputs: a plain run carries no CPU baseline and starts no PMC
pass, and the dump holds what the timed path left in its output buffers (whole, or a fixed sample of rows
within the byte budget), in the run's own precision."""
import json
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, str(ROOT))
import bench  # noqa: E402


class _Fake(bench.Workload):
    def __init__(self, arrays):
        self.arrays = arrays

    def outputs(self):
        return self.arrays


def test_plain_run_defaults():
    a = bench.parse(["--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert a.full is False and a.dump_outputs == "" and bench.want_pmc(a) is False
    assert bench.parse(["--full"]).full is True


def test_dump_outputs_whole(tmp_path):
    torch = pytest.importorskip("torch")
    a = torch.arange(12, dtype=torch.float64).view(4, 3)
    b = torch.arange(10, dtype=torch.float32).view(5, 2)
    bench.dump_outputs(_Fake([("a", a), ("b", b)]), str(tmp_path / "d"), 0, 1)
    ga, gb = np.load(tmp_path / "d" / "a.npy"), np.load(tmp_path / "d" / "b.npy")
    assert ga.dtype == np.float64 and gb.dtype == np.float32
    assert np.array_equal(ga, a.numpy()) and np.array_equal(gb, b.numpy())
    bench.dump_outputs(_Fake([("a", a)]), str(tmp_path / "d"), 1, 2)
    assert np.array_equal(np.load(tmp_path / "d" / "rank1_a.npy"), a.numpy())


def test_dump_outputs_sample_is_fixed_and_within_budget(tmp_path, monkeypatch):
    torch = pytest.importorskip("torch")
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4096)
    g = torch.Generator().manual_seed(3)
    a = torch.randn(1000, 16, dtype=torch.float64, generator=g)  # 128000 B
    b = torch.randn(37, 8, dtype=torch.float32, generator=g)     # 1184 B
    for d in ("x", "y"):
        bench.dump_outputs(_Fake([("a", a), ("b", b)]), str(tmp_path / d), 0, 1)
    xa, xb = np.load(tmp_path / "x" / "a.npy"), np.load(tmp_path / "x" / "b.npy")
    assert np.array_equal(xa, np.load(tmp_path / "y" / "a.npy")) and np.array_equal(xb, np.load(tmp_path / "y" / "b.npy"))
    assert 0 < xa.shape[0] < 1000 and xa.shape[1] == 16 and 0 < xb.shape[0] <= 37 and xb.shape[1] == 8
    assert xa.nbytes + xb.nbytes <= 4096
    full = {r.tobytes() for r in a.numpy()}
    assert len({r.tobytes() for r in xa}) == xa.shape[0] and all(r.tobytes() in full for r in xa)  # distinct whole rows


@pytest.mark.gpu
def test_plain_bench_line_and_dump_c2(gpu_session, tmp_path, capsys):
    """A plain run of C2 (4096 x 1024 fp64 Hann) with --dump-outputs: the line's contract fields, no CPU baseline,
    and the dumped spectra at the oracle's bar (1e-10) on the first, last and a spread of windows of the same
    seeded series."""
    torch = pytest.importorskip("torch")
    import oracle
    from wavespec_amd import synth
    d = tmp_path / "dump"
    assert bench.main(["--gpus", "1", "--config", "c2", "--steps", "3", "--warmup", "1", "--dump-outputs", str(d)]) == 0
    line = json.loads([l for l in capsys.readouterr().out.splitlines() if l.startswith("{")][-1])
    assert line["metric"] == "FFT-windows/sec" and line["unit"] == "windows/s" and line["higher_is_better"] is True
    assert line["dtype"] == "f64" and line["steps"] == 3 and line["warmup"] == 1
    assert line["ms_per_step"] > 0 and line["value"] == pytest.approx(4096 / (line["ms_per_step"] * 1e-3), rel=1e-9)
    assert line["cpu_baseline"] is None and line["cpu_baseline_all_cores"] is None
    assert sorted(p.name for p in d.iterdir()) == ["out.npy"]
    got = np.load(d / "out.npy")
    c = synth.CONFIGS["c2"]
    n, w = c["n"], c["windows"]
    assert got.dtype == np.float64 and got.shape == (w, n // 2)
    s = synth.random_walk_torch(n * w, c["seed"], torch.device("cuda", 0)).cpu().numpy().reshape(w, n)
    idx = np.r_[0, 1, w - 2, w - 1, np.arange(7, w, 509)]
    want = np.stack([oracle.window_spectrum(x, "none", "hann") for x in s[idx]])
    assert oracle.rel_err(got[idx], want) <= 1e-10
