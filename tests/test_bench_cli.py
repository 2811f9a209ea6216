"""bench.py's command line: a plain run prints the headline alone, --full adds the roofline, the
checks and the CPU baselines, --dump-outputs writes the arrays of the last timed step."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup"}
FULL_ONLY = {"roofline", "qps_per_step", "all_optimal", "cpu_baseline", "cpu_baseline_1core"}
n, N, S = 4, 5, 50  # 50 platoons over the default 3 streams: handles of 16, 17 and 17 platoons
SMALL = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--n", str(n), "--N", str(N), "--platoons", str(S)]


def run_bench(args: list) -> dict:
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True,
                       text=True, timeout=240)
    assert r.returncode == 0, r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_dump_outputs_types_and_seeded_sample(tmp_path, monkeypatch):
    """Tensors of the handles are joined in order; float64 stays, int8 becomes float32, int32 float64,
    entries that are no tensors are left out.  Past the size limit every array keeps the same seeded
    rows (ascending), within the limit, identically from call to call."""
    import torch

    import bench

    idx = torch.arange(10, dtype=torch.int32)
    full = {"u": torch.stack([2.0 * idx.double(), -idx.double()], 1), "region": (idx % 3).to(torch.int8)[:, None],
            "status": idx}
    groups = [{**{k: v[:6] for k, v in full.items()}, "runs": [1]}, {**{k: v[6:] for k, v in full.items()}, "runs": []}]
    bench.dump_outputs(str(tmp_path / "a"), groups)
    assert sorted(os.listdir(tmp_path / "a")) == ["region.npy", "status.npy", "u.npy"]
    got = {k: np.load(tmp_path / "a" / f"{k}.npy") for k in full}
    assert got["u"].dtype == np.float64 and got["region"].dtype == np.float32 and got["status"].dtype == np.float64
    for k, v in full.items():
        assert np.array_equal(got[k], v.numpy().astype(got[k].dtype))

    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 100)  # the arrays hold 160 + 40 + 80 bytes
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), groups)
    b = {k: np.load(tmp_path / "b" / f"{k}.npy") for k in full}
    assert 0 < sum(a.nbytes for a in b.values()) <= 100
    rows = b["status"].astype(int)
    assert len(rows) >= 1 and np.all(np.diff(rows) > 0)
    for k, v in full.items():
        assert np.array_equal(b[k], v.numpy()[rows].astype(b[k].dtype))
        assert np.array_equal(b[k], np.load(tmp_path / "c" / f"{k}.npy"))


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_last_step(gpu_available, tmp_path):
    """A plain run: the headline fields with the requested steps, nothing of --full, and the dumped
    arrays are the solver's answers to the bench's own inputs (integers exact, cost to 1e-9
    relative, u and x to 1e-6: the parity bars of the suite)."""
    import torch

    import bench
    from hvp import tables
    from hvp.models import PwaGearVehicle
    from hvp.solver import BatchSolver

    d = run_bench(SMALL + ["--dump-outputs", str(tmp_path / "d")])
    assert HEADLINE <= set(d) and not FULL_ONLY & set(d), sorted(d)
    assert d["steps"] == 2 and d["warmup"] == 1 and d["unit"] == "platoon-timesteps/s" and d["dtype"] == "f64"
    assert d["higher_is_better"] is True and d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(S / (d["ms_per_step"] * 1e-3), rel=1e-9)

    params, roles = bench.make_inputs(range(S), n, N)
    veh = PwaGearVehicle(800)
    solver = BatchSolver(tables.problem(N), [tables.system_from_dict(veh.get_discrete_system(1), tables.gears_of(veh))])
    dev = torch.device("cuda", 0)
    ref = solver.solve_device(torch.zeros(S * n, dtype=torch.int32, device=dev), torch.from_numpy(roles).to(dev),
                              torch.from_numpy(params).to(dev))
    torch.cuda.synchronize()
    got = {k: np.load(tmp_path / "d" / f"{k}.npy") for k in ref}
    assert sum(a.nbytes for a in got.values()) <= 64e6
    for k in ("region", "gear", "status"):
        assert got[k].dtype in (np.float32, np.float64)
        assert np.array_equal(got[k], ref[k].cpu().numpy().astype(got[k].dtype)), k
    assert np.all(got["status"] == 0)
    cost = ref["cost"].cpu().numpy()
    assert got["cost"].dtype == np.float64 and np.all(np.abs(got["cost"] - cost) <= 1e-9 * np.maximum(1.0, np.abs(cost)))
    for k in ("u", "x"):
        assert got[k].dtype == np.float64 and got[k].shape == tuple(ref[k].shape)
        assert np.max(np.abs(got[k] - ref[k].cpu().numpy())) <= 1e-6, k


@pytest.mark.gpu
def test_full_run_adds_the_roofline_the_checks_and_the_cpu_baselines(gpu_available):
    d = run_bench(SMALL + ["--full", "--cpu-budget", "0.2"])
    assert HEADLINE | FULL_ONLY <= set(d), sorted(d)
    assert d["steps"] == 2 and d["all_optimal"] is True
    assert d["roofline"]["qp_ms_per_step"] > 0 and d["qps_per_step"] > 0
    assert d["cpu_baseline"]["value"] > 0 and d["cpu_baseline_1core"]["cores"] == 1
    assert d["value"] == pytest.approx(S / (d["ms_per_step"] * 1e-3), rel=1e-9)
