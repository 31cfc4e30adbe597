"""bench.py on the GPU at small sizes: a plain run prints the headline line only, `--steps` sets the number of timed fills
(more of them than the pool of pristine copies, so the fills run in rounds), `--dump-outputs` writes the last fill's output
-- equal to the oracle's fill of the same DEM, whole or at its seeded sample of cells -- and `--full` adds the rest."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from richdem_amd.synth import fractal_dem

pytestmark = pytest.mark.gpu

sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _bench(*args, timeout=600):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "RDGPU_BENCH_FORCE_SHARDED"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *args], capture_output=True, text=True,
                       env=env, cwd=ROOT, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


@pytest.mark.parametrize("size,steps", [(600, 3), (2100, bench.STEP_POOL + 3)])
def test_plain_run_steps_and_dumped_outputs(orc, tmp_path, size, steps):
    d = _bench("--size", str(size), "--steps", str(steps), "--warmup", "1", "--dump-outputs", str(tmp_path))
    assert d["steps"] == steps and d["warmup"] == 1 and d["n_gpus"] == 1
    assert d["unit"] == "Mcells/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["ms_per_step"] > 0 and d["value"] == pytest.approx(size * size / 1e3 / d["ms_per_step"], rel=0.01)
    for k in ("roofline", "kernels_ms_per_step", "stages", "end_to_end_host", "cpu_baseline"):
        assert k not in d, k                                      # --full's
    exp = orc.port.fill(fractal_dem(size, size, 3))               # bench.py's DEM: G(seed=3), the same generator on the host
    got = np.load(tmp_path / "filled_dem.npy")
    assert got.dtype == np.float32
    if size * size <= bench.DUMP_SAMPLE:
        assert not (tmp_path / "filled_dem_cells.npy").exists()
        assert np.array_equal(got, exp)
    else:
        cells = np.load(tmp_path / "filled_dem_cells.npy")
        # the seeded sample of cells: the same positions in every run (unique, sorted; collisions make it smaller)
        idx = np.unique(np.random.default_rng(bench.DUMP_SEED).integers(0, size * size, bench.DUMP_SAMPLE, dtype=np.int64))
        assert cells.dtype == np.float64 and np.array_equal(cells, idx.astype(np.float64)) and got.shape == idx.shape
        assert np.array_equal(got, exp.reshape(-1)[idx])


def test_full_run_carries_the_rest():
    d = _bench("--size", "3000", "--steps", "2", "--warmup", "1", "--full", "--cpu-sample", "300")
    assert d["steps"] == 2 and d["ms_per_step"] > 0
    assert d["roofline"]["bound"] == "hbm" and d["kernels_ms_per_step"]
    st = d["stages"]
    for k in ("fill", "d8_flow_directions", "directions_plus_flat_resolution", "d8_flow_accum", "resolve_flats_epsilon",
              "fa_d8", "dinf_flow_directions", "fa_tarboton", "priority_flood_epsilon", "priority_flood_flowdirs"):
        assert st[k]["ms"] > 0, k
    assert d["end_to_end_host"]["ms"] > 0 and d["cpu_baseline"]["value"] > 0
