"""bench.py's own multi-rank launcher: `python3 bench.py --gpus N` started without a torchrun environment
spawns its N ranks (one process per GPU, torch.distributed.run on 127.0.0.1) and rank 0 prints the line.

CPU: the launcher and the decomposition with --dry-run (gloo, no GPU touched). GPU: the real 2-rank bench
on the box's one card (DFMI_RCCL_SPLIT_HOSTS=1: RCCL over sockets), a functional check of the line, not a
scaling number."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT


def _run(args, timeout, extra_env=None):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env.update(extra_env or {})
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-3000:])
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout      # exactly one JSON line, from rank 0
    return json.loads(lines[0])


@pytest.mark.parametrize("n_gpus,layout", [(2, "2x1x1"), (4, "2x2x1")])
def test_bench_spawns_its_ranks_dry_run(n_gpus, layout):
    d = _run(["--gpus", str(n_gpus), "--n", "16", "--dry-run"], 240, {"DFMI_RCCL_SPLIT_HOSTS": "1"})
    assert d["n_gpus"] == n_gpus and d["scaling"] == "weak"
    assert layout in d["config"]["parallelism"]
    assert d["config"]["cells_total"] == n_gpus * 16 ** 3
    assert sorted(e["rank"] for e in d["ranks"]) == list(range(n_gpus))
    assert sorted(e["local_rank"] for e in d["ranks"]) == list(range(n_gpus))
    assert all(e["proc_faces"] > 0 for e in d["ranks"])   # every block has processor patches


def test_bench_single_gpu_dry_run_stays_in_process():
    d = _run(["--gpus", "1", "--n", "8", "--dry-run"], 120)
    assert d["n_gpus"] == 1 and d["config"]["parallelism"] == "single"


@pytest.mark.gpu
def test_bench_plain_run_prints_the_headline_and_dumps_its_outputs(tmp_path):
    """without --full: the headline fields only, --steps timed steps, and --dump-outputs writes the last
    step's state as float64 arrays of the mesh's own sizes (12^3 cells: below the sampling threshold). Three
    runs side by side: the same arguments twice give the same files bit for bit, and --steps 1 instead of
    --steps 3 gives another state, so the dump is taken after the timed steps and --steps sets their number."""
    from concurrent.futures import ThreadPoolExecutor
    import numpy as np
    runs = {"a": "3", "b": "3", "c": "1"}
    with ThreadPoolExecutor(len(runs)) as ex:
        lines = dict(zip(runs, ex.map(lambda kv: _run(["--gpus", "1", "--n", "12", "--steps", kv[1], "--warmup", "1",
                                                       "--dump-outputs", str(tmp_path / kv[0])], 120), runs.items())))
    d = lines["a"]
    assert d["metric"].startswith("cell-updates/s") and d["unit"] == "cell-updates/s" and d["dtype"] == "f64"
    assert d["higher_is_better"] is True and d["steps"] == 3 and d["warmup"] == 1 and d["finite"] is True
    assert d["ms_per_step"] > 0 and d["value"] == pytest.approx(12 ** 3 / (d["ms_per_step"] * 1e-3))
    assert not {"roofline", "rooflines", "cpu_baseline", "other_configs", "other_schemes"} & set(d)
    C, F = 12 ** 3, 3 * 12 * 12 * 11              # the periodic faces are cyclic patches, not internal faces
    shapes = {"T": (C,), "p": (C,), "rho": (C,), "he": (C,), "U": (3, C), "Y": (9, C), "phi": (F,)}
    assert sorted(os.listdir(tmp_path / "a")) == sorted(k + ".npy" for k in shapes)
    got = {r: {k: np.load(tmp_path / r / (k + ".npy")) for k in shapes} for r in runs}
    for k, shape in shapes.items():
        a = got["a"][k]
        assert a.dtype == np.float64 and a.shape == shape and np.isfinite(a).all(), k
        assert np.array_equal(a, got["b"][k]), k            # same arguments: the same output
        assert not np.array_equal(a, got["c"][k]), k        # two more timed steps: every field has moved
    assert got["a"]["T"].min() > 200.0 and got["a"]["rho"].min() > 0.0


def test_dump_sample_is_fixed_and_within_budget(tmp_path):
    """the sampled indices of a large mesh are the same on every call, sorted and unique; 16 species at the
    sample size stay under the 64 MB a dump may take"""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    taken = {}

    class Ctx:
        def get_field(self, name, shape):
            return np.arange(shape[-1], dtype=np.float64) * np.ones(shape)

    class M:
        n_cells, n_faces = 3 * bench.DUMP_SAMPLE, 9 * bench.DUMP_SAMPLE
    for run in (0, 1):
        bench.dump_outputs(Ctx(), M, 16, str(tmp_path / str(run)))
        taken[run] = {f: np.load(tmp_path / str(run) / f) for f in os.listdir(tmp_path / str(run))}
    assert sum(a.nbytes for a in taken[0].values()) <= 64e6
    for f, a in taken[0].items():
        assert np.array_equal(a, taken[1][f]) and a.shape[-1] == bench.DUMP_SAMPLE, f
    assert (np.diff(taken[0]["T.npy"]) > 0).all() and np.array_equal(taken[0]["U.npy"][2], taken[0]["T.npy"])


@pytest.mark.gpu
def test_bench_two_ranks_on_one_card():
    """the same command the driver runs for N = 2, on one GPU: both ranks step the decomposed box over RCCL"""
    d = _run(["--gpus", "2", "--n", "16", "--steps", "3", "--warmup", "1", "--full", "--roof-steps", "1",
              "--alt-steps", "0", "--no-cpu", "--no-flame"], 280, {"DFMI_RCCL_SPLIT_HOSTS": "1"})
    assert d["n_gpus"] == 2 and "2x1x1" in d["config"]["parallelism"]
    assert d["finite"] and d["value"] > 0
    assert d["ms_per_step_median"] > 0
    assert "comm" in d and d["comm"]["points"]
