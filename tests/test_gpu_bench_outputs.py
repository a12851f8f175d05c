"""
bench.py as a plain run on the GPU (`--gpus 1 --steps K --warmup W`, no --full): one line without what --full adds, and
`--dump-outputs DIR` writing what the timed path computed in its last step.  The dumped edges of the stream are checked against
the float64 oracle over the same seeded input (bench.make_input), the seeded sample against the edges where they overlap.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import dd_oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS, F_OFF, NTAPS, LOG2N, W = 2400000, 25000.0, 255, 22, 8192
TOL = 2e-5          # as tests/test_gpu_fullsize.py: the bench input keeps |y[n] conj y[n-1]| far from zero


@pytest.mark.timeout(150)
def test_plain_run_dumps_what_the_timed_path_computed(tmp_path):
    torch = pytest.importorskip("torch")
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "DD_BENCH_STUB", "DD_BENCH_ONE_DEVICE", "DD_BENCH_FORCE_DIST"):
        env.pop(k, None)
    d = str(tmp_path / "dump")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--log2n", str(LOG2N), "--steps", "5",
                        "--warmup", "2", "--ramp-ms", "5", "--dump-outputs", d], capture_output=True, text=True, env=env, cwd=ROOT, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    j = json.loads(lines[0])
    n = 1 << LOG2N
    assert j["steps"] == 5 and j["warmup"] == 2 and j["ms_per_step"] > 0 and j["value"] > 0
    assert j["config"]["samples_per_gpu"] == n and j["config"]["kernel"] == "k_chain_cos1k" and j["data"] == "synthetic"
    assert not [k for k in ("first_step_ms", "cold_ms_per_step", "steady_check", "output_rms_rad", "side") if k in j["extra"]]
    assert "cpu_baseline" not in j

    a = {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}
    cnt = n - 1                                                         # the stream's first chunk owns one output fewer (quirk Q3)
    assert a["fm_angle_count"].tolist() == [cnt]
    head, tail, smp = a["fm_angle_head"], a["fm_angle_tail"], a["fm_angle_sample"]
    idx = a["fm_angle_sample_index"].astype(np.int64)
    E = len(head)
    assert head.dtype == tail.dtype == smp.dtype == np.float32 and len(tail) == E == 1 << 16
    assert len(idx) == len(smp) and np.all(np.diff(idx) > 0) and idx[-1] < cnt
    lo, hi = idx < E, idx >= cnt - E
    assert lo.any() and hi.any()
    assert np.array_equal(smp[lo], head[idx[lo]]) and np.array_equal(smp[hi], tail[idx[hi] - (cnt - E)])
    assert np.all(np.isfinite(smp)) and 0.005 < float(np.sqrt(np.mean(smp.astype(np.float64) ** 2))) < 0.02   # the 1 kHz tone

    # both ends against the float64 oracle (windows as tests/test_gpu_fullsize.py forms them)
    import bench
    x = bench.make_input(torch, n, 0, torch.device("cuda", 0), 1235)      # rank 0's input, the bench's seed
    taps = np.ascontiguousarray(0.54 - 0.46 * np.cos(2.0 * np.pi * np.arange(NTAPS) / (NTAPS - 1)))
    for w0, edge, e0 in ((0, head, 0), (n - W, tail, cnt - E)):
        h0 = max(0, w0 - (NTAPS - 1) - 1)
        xs = x[h0:w0 + W].cpu().numpy().astype(np.float32)
        y = O.nco((xs[:, 0] + 1j * xs[:, 1]).astype(np.complex64), F_OFF, FS, h0)
        if h0 == 0:
            y = O.FilterState(taps).applyOn(y)                           # stream start: history of ones (Q1)
        else:
            y = O.lfilter_fir(taps, y, None)[NTAPS - 1:]
            h0 += NTAPS - 1
        a_ref, _ = O.fm_demod(y, None)                                   # a_ref[i] pairs global samples h0+i+1, h0+i: output h0+i
        got = edge[h0 - e0:h0 - e0 + len(a_ref)].astype(np.float64)
        assert len(got) == len(a_ref) >= W - 1, (w0, len(got), len(a_ref))
        err = np.abs(np.angle(np.exp(1j * (got - a_ref))))
        assert np.max(err) < TOL, (w0, float(np.max(err)))
