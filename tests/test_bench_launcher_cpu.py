"""bench.py's own rank fan-out (`--gpus N` without an external launcher), driven on CPU: the parent starts
`torch.distributed.run` BEFORE torch / HIP are imported, the ranks meet over gloo, deal the raster, all-reduce the twi
partials, the slowest rank's time and the unit counts, and rank 0's single JSON line comes back through the parent.
`--stub` replaces the solver (which needs a GPU) by a stand-in; launcher, partition and collectives are the code under
test.  The line is flagged "stub": true so that it can never be mistaken for a measurement."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np

from microclimf_amd import synthetic

ROOT = Path(__file__).resolve().parent.parent


def _run(*argv, timeout=300):
    p = subprocess.run([sys.executable, str(ROOT / "bench.py"), *argv], capture_output=True, text=True, timeout=timeout,
                       cwd=str(ROOT))
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout            # exactly ONE JSON line on stdout
    return json.loads(lines[0])


def _valid(rows, cols):
    vegp, _, _ = synthetic.rasters(rows, cols, 0, rows)
    return int((~np.isnan(vegp["hgt"])).sum())


def test_defaults_are_the_headline_config():
    sys.path.insert(0, str(ROOT))
    import bench
    a = bench.parse([])
    assert (a.config, a.rows, a.cols, a.terrain, a.scaling, a.gpus, a.tsteps) == (2, 4096, 4096, "device", "weak", 1, 8760)
    a = bench.parse(["--config", "3"])
    assert (a.rows, a.cols, a.terrain, a.scaling, a.share) == (8192, 8192, "device", "strong", 8)
    a = bench.parse(["--config", "1", "--rows", "512"])
    assert (a.rows, a.cols, a.terrain) == (512, 1024, "random")


def test_parent_does_not_import_torch_before_launching():
    code = ("import sys; sys.argv=['bench.py']; import bench; bench.parse(['--gpus','2']); "
            "assert 'torch' not in sys.modules, 'torch imported at module level'")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=str(ROOT))


def test_gpus_2_starts_two_ranks_weak():
    line = _run("--gpus", "2", "--stub", "--config", "1", "--rows", "40", "--cols", "16", "--steps", "2", "--warmup", "0")
    assert line["n_gpus"] == 2 and line["stub"] is True and line["scaling"] == "weak"
    # weak scaling: 40 rows PER rank; the two blocks are rows 0..39 and 40..79 of ONE 80-row raster (seeded by global index)
    assert line["config"]["valid_cells"] == _valid(80, 16)
    _, soilc, _ = synthetic.rasters(80, 16, 0, 80)
    assert abs(line["config"]["twi_mean"] - float(np.mean(np.log(soilc["twi"]) / 1.5))) < 1e-12


def test_gpus_2_strong_share_of_eight_blocks():
    line = _run("--gpus", "2", "--stub", "--config", "3", "--rows", "80", "--cols", "16", "--steps", "1", "--warmup", "0")
    assert line["n_gpus"] == 2 and line["scaling"] == "strong"
    # 80 rows in 8 blocks of 10; ranks 0 and 1 hold rows 0..19
    vegp, _, _ = synthetic.rasters(20, 16, 0, 80)
    assert line["config"]["valid_cells"] == int((~np.isnan(vegp["hgt"])).sum())


def test_single_rank_needs_no_launcher():
    line = _run("--gpus", "1", "--stub", "--config", "1", "--rows", "24", "--cols", "8", "--steps", "1", "--warmup", "0")
    assert line["n_gpus"] == 1 and line["config"]["valid_cells"] == _valid(24, 8)


def test_plain_run_is_the_default_and_full_adds_the_rest():
    sys.path.insert(0, str(ROOT))
    import bench
    a = bench.parse(["--steps", "7"])
    assert a.steps == 7 and not a.full and a.dump_outputs is None
    a = bench.parse(["--full", "--dump-outputs", "out"])
    assert a.full and a.dump_outputs == "out"


def test_inputs_built_in_row_slices_are_those_of_one_call():
    """bench.py builds a rank's block in row slices on a thread pool: bit for bit the arrays of one synthetic.workload call
    (column-major as that returns them), and the DTM of one synthetic.rasters call — over a halo-extended block too"""
    sys.path.insert(0, str(ROOT))
    import bench
    args = bench.parse(["--config", "1", "--tsteps", "48"])
    rows, cols, row0, rows_total = 77, 23, 40, 300
    got, cpos, terrain_s = bench.build_workload(args, synthetic, 0, 1, 0, rows, cols, row0, rows_total, 48, False, None, True)
    want = synthetic.workload(rows, cols, 48, reqhgt=args.reqhgt, row0=row0, rows_total=rows_total, start_doy=1)
    assert cpos is None and terrain_s is None and set(got) == set(want)
    for g in ("vegp", "soilc"):
        assert list(got[g]) == list(want[g])
        for k, v in want[g].items():
            assert got[g][k].flags.f_contiguous and np.array_equal(got[g][k], v, equal_nan=True), (g, k)
    for g in ("climdata", "pointm", "obstime"):
        for k, v in want[g].items():
            assert np.array_equal(got[g][k], v), (g, k)
    assert all(got[k] == want[k] for k in want if k not in ("vegp", "soilc", "climdata", "pointm", "obstime"))
    dtm = bench.rows_in_threads(lambda r0, r1: {"dtm": synthetic.rasters(r1 - r0, cols, row0 - 9 + r0, rows_total)[2]}, rows + 17)
    assert np.array_equal(dtm["dtm"], synthetic.rasters(rows + 17, cols, row0 - 9, rows_total)[2])


def test_dump_samples_only_cells_that_hold_data(tmp_path):
    """--dump-outputs on a stand-in plan whose NA cells read NaN: the sample is drawn from the cells that hold data only, the
    same for the same raster, the days in day order whichever ring slot holds them, the files within the budget"""
    sys.path.insert(0, str(ROOT))
    import bench

    class Plan:
        rows, cols = 300, 200

        def __init__(self, na):
            self.na = na

        def fetch_cells(self, slot, var, step0, nsteps, cells):
            v = np.repeat((100.0 * slot + step0 // 24 + cells / 1e6)[None, :], nsteps, axis=0).T
            v[self.na[cells]] = np.nan
            return v

    na = synthetic.uniform(31, np.arange(300 * 200)) < 0.2
    resident = {(1, 0): 10, (1, 1): 11, (0, 0): 12}               # slot 1 holds days 10, 11; slot 0 day 12
    bench.dump_outputs(Plan(na), resident, tmp_path / "a", ~na, budget=2e6)
    bench.dump_outputs(Plan(na), resident, tmp_path / "b", ~na, budget=2e6)
    files = sorted(tmp_path.glob("a/*.npy"))
    assert len(files) == 10 and sum(f.stat().st_size for f in files) <= 2e6 + 10 * 256
    for f in files:
        a = np.load(f)
        assert a.shape[1] == 72 and 0 < a.shape[0] < (~na).sum() and np.isfinite(a).all(), f.name
        assert np.array_equal(a[:, ::24].round(), np.tile([100.0, 101.0, 0.0], (a.shape[0], 1)))
        assert np.array_equal(a, np.load(tmp_path / "b" / f.name))
