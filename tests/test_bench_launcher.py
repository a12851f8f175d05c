"""
bench.py's launcher path on CPU: `python bench.py --gpus 2` (no WORLD_SIZE) must start two ranks under
torch.distributed.run, never import torch in the launcher itself, and relay rank 0's single JSON line
with n_gpus = 2.  DD_BENCH_STUB=1 swaps the HIP engine for a do-nothing stand-in and RCCL for gloo
(the line it prints is marked `data: "stub"`): what is tested is the launch / barrier / max-over-ranks /
gather plumbing, not a measurement.
"""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(extra_args, env_extra=None, timeout=240):
    env = dict(os.environ)
    env["DD_BENCH_STUB"] = "1"
    env.pop("WORLD_SIZE", None)
    env.pop("RANK", None)
    env.pop("LOCAL_RANK", None)
    env.update(env_extra or {})
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + extra_args, capture_output=True, text=True,
                       env=env, timeout=timeout, cwd=ROOT)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    return r, lines


@pytest.mark.timeout(300)
def test_gpus_2_launches_two_ranks_and_prints_one_line():
    r, lines = _run(["--gpus", "2", "--steps", "4", "--warmup", "1", "--ramp-ms", "2", "--full"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert len(lines) == 1, r.stdout
    j = json.loads(lines[0])
    assert j["n_gpus"] == 2 and j["steps"] == 4 and j["warmup"] == 1
    assert j["data"] == "stub" and j["config"]["kernel_path"] == "stub"
    assert j["scaling"] == "weak" and j["higher_is_better"] is True
    assert len(j["extra"]["kernel_ms_per_rank"]) == 2
    # gather leg: rank 0 of the stream contributes n-1 outputs (quirk Q3), every other rank n
    assert j["extra"]["gathered_outputs"] == 2 * j["config"]["samples_per_gpu"] - 1
    assert "with_all_gather_MSamples_per_s" in j["extra"] and "all_gather_ms_per_step" in j["extra"]      # without --gather
    assert j["extra"]["world_size_seen"] == 2 and j["extra"]["backend"] == "gloo"
    assert "cpu_baseline" not in j                      # rank 0 at N = 1 only


@pytest.mark.timeout(300)
def test_no_gather_skips_the_collective_leg():
    r, lines = _run(["--gpus", "2", "--steps", "3", "--warmup", "1", "--ramp-ms", "2", "--full", "--no-gather"])
    assert r.returncode == 0, r.stderr[-2000:]
    j = json.loads(lines[0])
    assert "with_all_gather_MSamples_per_s" not in j["extra"] and j["extra"]["world_size_seen"] == 2


@pytest.mark.timeout(120)
def test_short_node_gets_one_clear_line():
    """--gpus 4 on a node that shows fewer GPUs (this container shows none): the launcher probes the device count in a
    throw-away child and leaves with one line and a non-zero code, before building or starting any rank"""
    env = dict(os.environ)
    for k in ("DD_BENCH_STUB", "DD_BENCH_ONE_DEVICE", "WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    env["HIP_VISIBLE_DEVICES"] = ""
    env["CUDA_VISIBLE_DEVICES"] = ""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4"], capture_output=True, text=True, env=env, timeout=100, cwd=ROOT)
    assert r.returncode == 2, (r.returncode, r.stderr[-500:])
    msg = [ln for ln in r.stderr.splitlines() if ln.startswith("bench.py:")]
    assert len(msg) == 1 and "--gpus 4" in msg[0] and "visible" in msg[0], r.stderr[-500:]
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]


@pytest.mark.timeout(120)
def test_single_rank_runs_in_process():
    r, lines = _run(["--steps", "3", "--warmup", "1", "--ramp-ms", "1", "--no-cpu-baseline", "--full"])
    assert r.returncode == 0, r.stderr[-2000:]
    j = json.loads(lines[-1])
    assert j["n_gpus"] == 1 and "kernel_ms_per_rank" not in j["extra"]
    assert j["extra"]["steady_check"]["steps"] >= 3 and j["extra"]["cold_ms_per_step"] > 0


def test_launcher_does_not_import_torch_or_hip():
    """the parent of the ranks must stay clear of the GPU: it may not import torch or load the extension"""
    code = (
        "import sys, os; sys.argv=['bench.py','--gpus','2']; os.environ.pop('WORLD_SIZE', None)\n"
        "import bench, subprocess\n"
        "calls=[]\n"
        "class P:\n"
        "    stdout=[]\n"
        "    def wait(self): return 0\n"
        "subprocess.Popen=lambda cmd, **k: (calls.append(cmd), P())[1]\n"
        "subprocess.run=lambda cmd, **k: type('R',(),{'returncode':0,'stdout':'8\\n'})()\n"
        "try:\n"
        "    bench.main()\n"
        "except SystemExit as e:\n"
        "    assert e.code == 0, e.code\n"
        "assert 'torch' not in sys.modules and 'directdemod_amd' not in sys.modules, sorted(m for m in sys.modules if 'torch' in m)[:5]\n"
        "cmd=calls[0]\n"
        "assert '-m' in cmd and 'torch.distributed.run' in cmd and '--nproc-per-node=2' in cmd and '127.0.0.1' in cmd, cmd\n"
        "assert cmd[-2:] == ['--gpus','2'], cmd\n"
        "print('ok')\n")
    env = dict(os.environ)
    env.pop("DD_BENCH_STUB", None)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, env=env, timeout=60)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-2000:]


def test_the_drivers_8_gpu_command_line_parses_and_keeps_the_contract():
    """The scaling record is the driver's to measure (`python -m torch.distributed.run --nproc-per-node 8 ... bench.py --gpus 8
    --steps K --warmup W`); what can be checked here is that this command line parses to the C2 shard per rank, that the
    launcher would pass every argument through unchanged, and that `extra.rccl_init_s` (rendezvous + first collective) is part
    of a multi-rank line."""
    sys.path.insert(0, ROOT)
    import bench
    args = bench.parse_args(["--gpus", "8", "--steps", "20", "--warmup", "5"])
    assert (args.gpus, args.steps, args.warmup, args.log2n) == (8, 20, 5, 26)
    assert args.steady_ms >= 6000 and not args.no_gather
    assert not args.full and args.dump_outputs is None                  # a plain run by default
    args = bench.parse_args(["--gpus", "8", "--log2n", "26", "--steps", "20", "--warmup", "5", "--no-gather"])
    assert args.log2n == 26 and args.no_gather
    with pytest.raises(SystemExit):
        bench.parse_args(["--gpus", "eight"])
    r, lines = _run(["--gpus", "2", "--steps", "3", "--warmup", "1", "--ramp-ms", "2"])
    assert r.returncode == 0 and len(lines) == 1, r.stderr[-2000:]
    j = json.loads(lines[0])
    assert 0 <= j["extra"]["rccl_init_s"] < 60 and j["extra"]["world_size_seen"] == 2
    assert "[bench] rank 0/2: init_process_group" in r.stderr


REQUIRED = {"metric": str, "value": float, "unit": str, "higher_is_better": bool, "dtype": str, "ms_per_step": float}
FULL_ONLY = ("first_step_ms", "cold_ms_per_step", "steady_check", "output_rms_rad", "side",
             "with_all_gather_MSamples_per_s", "all_gather_ms_per_step", "gathered_outputs")


def _npy(d):
    import numpy as np
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


@pytest.mark.timeout(120)
def test_plain_run_times_its_steps_and_nothing_else():
    """a plain run: warm-up, the --steps timed steps, the line -- none of what --full adds, and the headline fields as before"""
    r, lines = _run(["--steps", "7", "--warmup", "2", "--ramp-ms", "0"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert len(lines) == 1, r.stdout
    j = json.loads(lines[0])
    for k, t in REQUIRED.items():
        assert isinstance(j[k], t), (k, j.get(k))
    assert j["steps"] == 7 and j["warmup"] == 2 and j["higher_is_better"] is True and j["dtype"] == "f32"
    assert j["ms_per_step"] >= 0.5                                     # the stand-in step sleeps 0.5 ms
    n = j["config"]["samples_per_gpu"]
    assert abs(j["value"] - n / (j["ms_per_step"] * 1e3)) <= 0.02 * j["value"] + 0.1     # one interval behind both figures
    assert not [k for k in FULL_ONLY if k in j["extra"]] and "cpu_baseline" not in j


@pytest.mark.timeout(120)
def test_dump_outputs_single_rank(tmp_path):
    """--dump-outputs DIR: float32 / float64 .npy files of the last timed step's output, the same from run to run"""
    import numpy as np
    got = []
    for i in range(2):
        d = str(tmp_path / ("run%d" % i))
        r, lines = _run(["--steps", "2", "--warmup", "0", "--ramp-ms", "0", "--dump-outputs", d])
        assert r.returncode == 0 and len(lines) == 1, r.stderr[-2000:]
        got.append(_npy(d))
    a = got[0]
    assert sorted(a) == ["fm_angle_count", "fm_angle_head", "fm_angle_sample", "fm_angle_sample_index", "fm_angle_tail"]
    cnt = 4096 - 1                                                     # stand-in shard: 2^12 samples, the stream's first owns one output fewer
    assert a["fm_angle_count"].dtype == np.float64 and a["fm_angle_count"].tolist() == [cnt]
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert len(a["fm_angle_head"]) == len(a["fm_angle_tail"]) == cnt    # shorter than DUMP_EDGE: the whole output at both ends
    assert np.array_equal(a["fm_angle_sample_index"], np.arange(cnt, dtype=np.float64))
    assert all(np.array_equal(a[k], got[1][k]) for k in a)


@pytest.mark.timeout(300)
def test_plain_two_ranks_dump_per_rank_and_skip_the_gather_leg(tmp_path):
    import numpy as np
    d = str(tmp_path / "dump")
    r, lines = _run(["--gpus", "2", "--steps", "3", "--warmup", "1", "--ramp-ms", "2", "--dump-outputs", d])
    assert r.returncode == 0 and len(lines) == 1, r.stderr[-2000:]
    j = json.loads(lines[0])
    assert j["n_gpus"] == 2 and not [k for k in FULL_ONLY if k in j["extra"]]
    a = _npy(d)
    assert sorted(a) == sorted("rank%d_fm_angle_%s" % (r_, k) for r_ in (0, 1) for k in ("count", "head", "sample", "sample_index", "tail"))
    n = j["config"]["samples_per_gpu"]
    assert a["rank0_fm_angle_count"].tolist() == [n - 1] and a["rank1_fm_angle_count"].tolist() == [n]
    assert np.all(a["rank0_fm_angle_sample"] == 0.0) and np.all(a["rank1_fm_angle_sample"] == 1.0)     # the stand-in's output is its rank


def test_dump_outputs_sample_is_fixed_and_within_64_MB(tmp_path):
    """the sampling path (outputs beyond DUMP_SAMPLE) on a host tensor standing in for a full 2^26-sample shard's output"""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    n = 1 << 26

    class Eng:
        pass
    eng = Eng()
    eng.torch = torch
    out = torch.arange(n, dtype=torch.float32) * 1e-7
    eng.shard_output = lambda: (out, n - 1)
    sizes = []
    for world in (1, 8):
        for i in range(2):
            d = str(tmp_path / ("w%d_%d" % (world, i)))
            bench.dump_outputs(eng, d, 0, world)
            sizes.append(sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)) * (world if world > 1 else 1))
        pre = "rank0_" if world > 1 else ""
        a, b = (_npy(str(tmp_path / ("w%d_%d" % (world, i)))) for i in range(2))
        assert all(np.array_equal(a[k], b[k]) for k in a)
        idx = a[pre + "fm_angle_sample_index"]
        assert idx.dtype == np.float64 and np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < n - 1
        assert len(idx) > 0.9 * bench.DUMP_SAMPLE / world
        assert np.array_equal(a[pre + "fm_angle_sample"], out.numpy()[idx.astype(np.int64)])
        assert np.array_equal(a[pre + "fm_angle_tail"], out.numpy()[n - 1 - bench.DUMP_EDGE:n - 1])
        assert np.array_equal(a[pre + "fm_angle_head"], out.numpy()[:bench.DUMP_EDGE])
    assert max(sizes) <= 64 << 20, sizes


def test_steps_below_one_are_refused():
    sys.path.insert(0, ROOT)
    import bench
    with pytest.raises(SystemExit):
        bench.parse_args(["--steps", "0"])


def test_a_finished_build_is_used_without_writing_to_the_tree(monkeypatch):
    """the benchmark may run as another user than the one whose build() left the library, in a tree it cannot write to: with
    the library there, the ranks' build check opens no file for writing, creates no directory and builds nothing"""
    import builtins
    sys.path.insert(0, ROOT)
    import bench
    import __graft_entry__ as ge

    def refuse(*a, **k):
        raise PermissionError("write into the tree: %r" % (a,))
    real_open = builtins.open
    monkeypatch.setattr(ge, "LIB", os.path.join(ROOT, "bench.py"))            # an existing file stands for the built library
    monkeypatch.setattr(ge, "build", refuse)
    monkeypatch.setattr(os, "makedirs", refuse)
    monkeypatch.setattr(builtins, "open", lambda f, mode="r", *a, **k:
                        refuse(f) if any(c in mode for c in "wax+") else real_open(f, mode, *a, **k))
    bench.build_once_per_node()
