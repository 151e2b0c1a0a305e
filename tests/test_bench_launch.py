"""bench.py's launch logic: `--gpus N` can never disagree with the ranks that run.
CPU-only: the decision function is pure, and the self-spawn path is exercised with a stub launcher module on PATH-less python."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (importing bench touches neither torch nor the GPU)


def test_single_gpu_plain_python_runs_in_process():
    a = bench.parse_args(["--gpus", "1"])
    assert bench.resolve_launch(a, ["--gpus", "1"], {}) == ("run", 0, 1, 0)


def test_multi_gpu_without_launcher_spawns_torchrun_child():
    argv = ["--gpus", "4", "--steps", "3", "--warmup", "1"]
    a = bench.parse_args(argv)
    kind, cmd = bench.resolve_launch(a, argv, {})
    assert kind == "spawn"
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nproc-per-node=4" in cmd and "--nnodes=1" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    i = cmd.index(os.path.join(ROOT, "bench.py"))
    assert cmd[i + 1:] == argv  # the child sees the same flags, so its --gpus equals its WORLD_SIZE


def test_under_launcher_world_must_equal_gpus():
    a = bench.parse_args(["--gpus", "8"])
    env = {"RANK": "3", "WORLD_SIZE": "8", "LOCAL_RANK": "3", "MASTER_ADDR": "127.0.0.1"}
    assert bench.resolve_launch(a, [], env) == ("run", 3, 8, 3)
    kind, msg = bench.resolve_launch(a, [], dict(env, WORLD_SIZE="4"))
    assert kind == "error" and "WORLD_SIZE=4" in msg
    a1 = bench.parse_args(["--gpus", "1"])
    kind, msg = bench.resolve_launch(a1, [], env)
    assert kind == "error"


def test_mismatch_exits_nonzero_before_touching_torch():
    env = dict(os.environ, RANK="0", WORLD_SIZE="2", LOCAL_RANK="0")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8"], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 2 and "must agree" in out.stderr and out.stdout.strip() == ""


def test_spawn_passes_the_childs_exit_code_on(tmp_path):
    """`python bench.py --gpus 2` with no RANK: the parent starts `python -m torch.distributed.run ...` as a child and returns its code.
    The child here is a stub package shadowing torch.distributed.run (no GPU in this container), which records its argv."""
    pkg = tmp_path / "torch" / "distributed"
    pkg.mkdir(parents=True)
    (tmp_path / "torch" / "__init__.py").write_text("")
    (pkg / "__init__.py").write_text("")
    (pkg / "run.py").write_text("import sys, json, os\nopen(os.environ['STUB_OUT'], 'w').write(json.dumps(sys.argv[1:]))\nsys.exit(7)\n")
    rec = tmp_path / "argv.json"
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    env.update(PYTHONPATH=str(tmp_path), STUB_OUT=str(rec))
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2"], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 7, (out.stdout, out.stderr)
    import json
    argv = json.loads(rec.read_text())
    assert "--nproc-per-node=2" in argv and argv[-4:] == ["--gpus", "2", "--steps", "2"]


def test_plain_run_measures_the_headline_only_and_full_keeps_the_rest():
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert not a.full and a.steps == 7 and a.warmup == 2
    assert a.no_prof and a.no_general_leg and a.no_secondary and a.no_cpu_baseline
    f = bench.parse_args(["--gpus", "1", "--full"])
    assert not (f.no_prof or f.no_general_leg or f.no_secondary or f.no_cpu_baseline) and f.secondary == "c3,c4,c5,sv"
    assert bench.parse_args(["--full", "--secondary", "c3", "--small-secondary"]).secondary == "c3"
    for extra in (["--secondary", "c3"], ["--small-secondary"]):
        with pytest.raises(SystemExit):
            bench.parse_args(extra)


def test_dump_outputs_writes_reals_within_the_budget(tmp_path):
    rng = np.random.default_rng(3)
    x = rng.standard_normal((8, 1000, 4))
    anc = rng.integers(0, 100, (8, 1000)).astype(np.int32)
    acc = np.array([1, 0, 1, 1, 0, 0, 1, 0], np.int32)
    bench.dump_outputs(str(tmp_path / "all"), dict(x=x, ancestors=anc), dict(accepted=acc), rank=0, world=1)
    got = {f[:-4]: np.load(tmp_path / "all" / f) for f in os.listdir(tmp_path / "all")}
    assert set(got) == {"x", "ancestors", "accepted"} and all(a.dtype in (np.float32, np.float64) for a in got.values())
    np.testing.assert_array_equal(got["x"], x)
    np.testing.assert_array_equal(got["ancestors"], anc)
    np.testing.assert_array_equal(got["accepted"], acc)
    # over the budget: the same seeded time steps of every trajectory, and their indices
    budget = 100_000
    for rep in ("s0", "s1"):
        bench.dump_outputs(str(tmp_path / rep), dict(x=x, ancestors=anc), dict(accepted=acc), rank=0, world=1, budget=budget)
    s0 = {f[:-4]: np.load(tmp_path / "s0" / f) for f in os.listdir(tmp_path / "s0")}
    s1 = {f[:-4]: np.load(tmp_path / "s1" / f) for f in os.listdir(tmp_path / "s1")}
    assert set(s0) == {"x", "ancestors", "accepted", "t_index"} and sum(a.nbytes for a in s0.values()) <= budget
    ti = s0["t_index"].astype(np.int64)
    assert np.all(np.diff(ti) > 0) and ti[-1] < 1000
    np.testing.assert_array_equal(s0["x"], x[:, ti])
    np.testing.assert_array_equal(s0["ancestors"], anc[:, ti])
    for k in s0:
        np.testing.assert_array_equal(s0[k], s1[k])
    # more than one rank: the files carry the rank
    bench.dump_outputs(str(tmp_path / "r"), dict(x=x), {}, rank=1, world=2)
    assert os.listdir(tmp_path / "r") == ["x_rank1.npy"]
