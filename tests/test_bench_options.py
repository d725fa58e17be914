"""bench.py's run options, on the host: ``--steps`` above the sampler's step count is split into whole pipeline runs (no step is
dropped), ``--dump-outputs`` writes float32 arrays inside its 64 MB budget and the same sample on every run, and ``--full``
exists."""
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_unit_iterations_cover_every_step():
    assert bench.unit_iterations(0, 50) == []
    assert bench.unit_iterations(20, 50) == [20]
    assert bench.unit_iterations(50, 50) == [50]
    assert bench.unit_iterations(120, 50) == [50, 50, 20]
    for n in range(0, 260, 7):
        units = bench.unit_iterations(n, 50)
        assert sum(units) == n and all(1 <= u <= 50 for u in units)


def test_dump_outputs_small_arrays_whole_in_their_shape(tmp_path):
    x = torch.arange(2 * 3 * 4 * 5, dtype=torch.uint8).view(2, 3, 4, 5)
    bench.dump_outputs(str(tmp_path / "d"), {"images": x})
    got = np.load(tmp_path / "d" / "images.npy")
    assert got.dtype == np.float32 and got.shape == (2, 3, 4, 5)
    assert np.array_equal(got, x.float().numpy())


def test_dump_outputs_large_arrays_as_a_fixed_sample_inside_the_budget(tmp_path):
    # one 4096^2 RGB image (the headline's output): 50 M elements, 201 MB as float32 -> a sample
    x = torch.randint(0, 256, (1, 3, 4096, 4096), dtype=torch.uint8, generator=torch.Generator().manual_seed(3))
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"images": x})
    a, b = np.load(tmp_path / "a" / "images.npy"), np.load(tmp_path / "b" / "images.npy")
    assert a.dtype == np.float32 and a.shape == (bench.DUMP_SAMPLE,)
    assert np.array_equal(a, b)                                    # same indices on every run
    assert os.path.getsize(tmp_path / "a" / "images.npy") < 64 * 2 ** 20
    idx = torch.randint(x.numel(), (bench.DUMP_SAMPLE,), generator=torch.Generator().manual_seed(0)).sort().values
    assert np.array_equal(a, x.reshape(-1)[idx].float().numpy())   # the documented sample


def test_cli_has_full_and_dump_outputs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "--full" in out.stdout and "--dump-outputs" in out.stdout
