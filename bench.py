#!/usr/bin/env python3
"""
bench.py -- headline benchmark of the DirectDemod hot path on MI355X.

Metric (BASELINE.json): IQ MSamples/s through 255-tap FIR + FM demod; % of HBM
roofline.  Workload = BASELINE.json configs[1] ("C2"):
  synthetic 2.4 MS/s complex64 IQ on the 8-bit source grid, device resident,
  N = 2^26 samples per GPU, commSignal.offsetFreq(25 kHz) NCO + filters.hamming(255)
  + demod_fm.demod, one chunk per step, output float32 radians (N-1 values).
A "step" = one pass of the fused hot path over the GPU's shard.  With --gpus N>1 the
stream is N shards of 2^26 samples, one rank per GPU: rank r re-filters the 256 samples
before its shard as a lead-in of the same launch (absolute-index state, no halo exchange)
and no collective sits on the data path (weak scaling).  With more than one rank, a --full run ALSO assembles the decoded
stream and times an RCCL all_gather of the decoded output per step (BASELINE north_star: "trivial RCCL/xGMI gather of
decoded output"), reported in "extra" (never in `value`); `--no-gather` skips that leg.

Plain run and --full.  A plain run (`bench.py --gpus 1 --steps K --warmup W`) does what its headline figure needs: set-up,
the clock pre-roll and the W warm-up steps, the K timed steps, the output dump if asked for, the JSON line.  `--full` adds
everything else the benchmark measures or checks: the process's first steps (`extra.first_step_ms`, `extra.cold_ms_per_step`),
the steady-state check (`extra.steady_check`), the output sanity figure (`extra.output_rms_rad`), the gather leg with more
than one rank, the side configurations (`extra.side`, N = 1) and the CPU baselines (`cpu_baseline`, N = 1);
`--no-side` / `--no-cpu-baseline` leave the last two out of a --full run.

Outputs.  `--dump-outputs DIR` writes what the timed path handed its caller in the last timed step -- the decoded angles of
the shard, float32 radians -- as DIR/<name>.npy right after the timed steps (before anything in a --full run reuses the
output buffer): the first and last DUMP_EDGE outputs, a fixed seeded sample of the outputs in between with its positions
(float64), and the output count.  The input is generated from fixed seeds, so two builds run with the same arguments can
be compared output for output.

Launching.  Under torch.distributed.run (WORLD_SIZE set) this process is one rank.  Started
plainly with --gpus N>1 it is the *launcher*: it builds the extension once (in a child
process), starts `python -m torch.distributed.run --nproc-per-node N ... bench.py <same
args>` as a child and relays its output (rank 0's JSON line); the launcher itself never
imports torch and never touches the GPU.

Timing.  `value` and `ms_per_step` are wall clock around the K timed steps (barrier +
device sync on both sides, max over ranks), and `roofline.achieved` / `roofline.frac` are computed from that
same interval (one basis for the whole line).  `roofline.kernel_ms_events` is HIP-event time on the
launch stream around the same K launches / K (one kernel launch per step), kept beside it.  20 steps are
only ~4 ms of device time, so a --full run also runs the same step for >= 100 ms right after the
timed region (`extra.steady_check`) and reports the process's first step (one-off costs) and the 19 after it,
before the pre-roll, in `extra.first_step_ms` / `extra.cold_ms_per_step`.

Prints ONE JSON line on rank 0.
"""
import argparse
import math
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0          # MI355X HBM3E spec peak (MI355X_MICROARCH.md)
BYTES_PER_SAMPLE = 12.0        # 8 B complex64 read + 4 B float32 written
FS = 2400000
F_OFFSET = 25000.0
NTAPS = 255


def make_input(torch, n, start, device, seed):
    """Input B of SURVEY.md 8(d): FM tone + noise rounded to the u8 source grid,
    generated on the device in float64 phase (synthetic)."""
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    out = torch.empty((n, 2), dtype=torch.float32, device=device)
    blk = 1 << 22
    for s0 in range(0, n, blk):
        s1 = min(n, s0 + blk)
        t = (torch.arange(s0 + start, s1 + start, device=device, dtype=torch.float64)) / FS
        ph = 2 * np.pi * 25e3 * t + 5.0 * torch.sin(2 * np.pi * 1e3 * t)
        ph = torch.remainder(ph, 2 * np.pi).to(torch.float32)
        re = 60.0 * torch.cos(ph) + 4.0 * torch.randn(s1 - s0, device=device, generator=g)
        im = 60.0 * torch.sin(ph) + 4.0 * torch.randn(s1 - s0, device=device, generator=g)
        out[s0:s1, 0] = torch.clamp(torch.round(re + 127.5), 0, 255) - 127.5
        out[s0:s1, 1] = torch.clamp(torch.round(im + 127.5), 0, 255) - 127.5
    return out


# ----------------------------------------------------------------------------- CPU baselines
def cpu_baseline_scipy(n):
    """The reference's own CPU arithmetic for this chain restated call for call (kind 'port', calls 'scipy'):
    comm.py:77 (np.exp NCO, in place on complex64), filters.py:45,69 (lfilter_zi + lfilter
    with carried zi), demod_fm.py:40-49 (np.angle of the conj-lagged product).  One thread."""
    import scipy.signal as ss
    from oracle import dd_oracle as O           # input generator only (cpu_baseline leg)
    x = O.grid_c64(O.synth_iq_fm(n, FS, 1235))
    b = ss.windows.hamming(NTAPS)
    a = [1]
    best = None
    for _ in range(2):
        sig = np.array(x)                                                    # commSignal ctor copies (comm.py:38)
        t0 = time.perf_counter()
        sig *= np.exp(-1.0j * 2.0 * np.pi * F_OFFSET * np.arange(0, n) / FS)
        zi = ss.lfilter_zi(b, a)
        y, zi = ss.lfilter(b, a, sig, zi=zi)
        ang = np.angle(y[1:] * np.conj(y[:-1]))
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    assert len(ang) == n - 1
    return {"value": round(n / best / 1e6, 3), "unit": "MSamples/s", "cores": 1, "kind": "port", "calls": "scipy",
            "sample": "2^%d samples of the same workload: np.exp NCO, scipy.signal.lfilter(b,[1],x,zi=lfilter_zi), "
                      "np.angle (comm.py:77, filters.py:45,69, demod_fm.py:40-49), best of 2, %.2f s"
                      % (int(np.log2(n)), best)}


def cpu_baseline_port(n):
    """The oracle's restatement of the same path (oracle/dd_oracle.py, np.convolve-based FIR), one thread."""
    from oracle import dd_oracle as O
    x = O.grid_c64(O.synth_iq_fm(n, FS, 1235))
    taps = O.win_hamming(NTAPS)
    best = None
    for _ in range(2):
        t0 = time.perf_counter()
        y = O.FilterState(taps).applyOn(O.nco(x, F_OFFSET, FS, 0))
        a, _ = O.fm_demod(y, None)
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    assert len(a) == n - 1
    return {"value": round(n / best / 1e6, 3), "unit": "MSamples/s", "cores": 1, "kind": "port", "calls": "oracle/dd_oracle.py (numpy)",
            "sample": "2^%d samples (numpy float64, best of 2, %.2f s)" % (int(np.log2(n)), best)}


def cpu_baseline_all_cores(timeout_s=240):
    """The SciPy path on every host core the process may use: one process per contiguous shard
    (tools/cpu_allcores.py, a child process that never touches the GPU), bounded by a timeout."""
    import signal
    import subprocess
    tool = os.path.join(ROOT, "tools", "cpu_allcores.py")
    try:
        p = subprocess.Popen([sys.executable, tool], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL,
                             start_new_session=True, text=True)
        try:
            out, _ = p.communicate(timeout=timeout_s)
        except subprocess.TimeoutExpired:
            os.killpg(p.pid, signal.SIGKILL)          # the child's own process group (its worker pool included)
            p.communicate()
            return {"error": "timed out after %d s" % timeout_s}
        if p.returncode != 0:
            return {"error": "exit code %d" % p.returncode}
        return json.loads(out.strip().splitlines()[-1])
    except Exception as e:                            # a reported baseline, never a reason to lose the bench line
        return {"error": repr(e)}


def cpu_baseline(n):
    res = cpu_baseline_scipy(n)
    res["host_cpus"] = os.cpu_count()
    res["usable_cpus"] = len(os.sched_getaffinity(0))
    res["oracle"] = cpu_baseline_port(n)
    res["all_cores"] = cpu_baseline_all_cores()
    return res


# ----------------------------------------------------------------------------- launcher (parent of the ranks)
def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def launch(n_gpus, argv):
    """--gpus N > 1 without WORLD_SIZE: build once, then run the N ranks under torch.distributed.run
    as a child process and relay what they print.  Nothing here imports torch or calls HIP (a process
    that has initialised the GPU must not fork/exec the ranks)."""
    import subprocess
    if not os.environ.get("DD_BENCH_STUB"):
        if not os.environ.get("DD_BENCH_ONE_DEVICE"):
            # how many GPUs does this node show?  Asked in a throw-away child (the launcher itself stays clear of torch
            # and HIP); a short node gets one clear line instead of a stack trace per rank
            r = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.device_count())"],
                               capture_output=True, text=True)
            try:
                seen = int((r.stdout or "").strip().splitlines()[-1])
            except (ValueError, IndexError):
                seen = -1
            if seen < n_gpus:
                sys.stderr.write("bench.py: --gpus %d asked for, %s GPU(s) visible on this node\n" % (n_gpus, seen if seen >= 0 else "no"))
                return 2
        r = subprocess.run([sys.executable, os.path.join(ROOT, "__graft_entry__.py")], stdout=subprocess.DEVNULL)
        if r.returncode != 0:
            raise SystemExit("bench.py: building the HIP extension failed (exit %d)" % r.returncode)
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")       # dmabuf IPC: RCCL needs it on this driver
    env.setdefault("OMP_NUM_THREADS", "1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=%d" % n_gpus,
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.abspath(__file__)] + list(argv)
    p = subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True, env=env)
    for line in p.stdout:
        sys.stdout.write(line)
        sys.stdout.flush()
    return p.wait()


def build_once_per_node():
    """Ranks started directly by torch.distributed.run: one rank at a time looks at the build (file lock),
    so N ranks never compile the same objects concurrently; a finished build is a few stat() calls and writes nothing (the
    tree may belong to another user than the one running the benchmark)."""
    import fcntl
    import __graft_entry__ as ge
    if os.path.exists(ge.LIB):
        return
    os.makedirs(os.path.join(ROOT, "build"), exist_ok=True)
    with open(os.path.join(ROOT, "build", ".lock"), "w") as lk:
        fcntl.flock(lk, fcntl.LOCK_EX)
        try:
            if not os.path.exists(ge.LIB):
                ge.build()
        finally:
            fcntl.flock(lk, fcntl.LOCK_UN)


# ----------------------------------------------------------------------------- engines
KERNEL_NAMES = {1: "k_chain_dense", 2: "k_chain_decim", 3: "k_chain_decim_p", 4: "k_chain_mfma_ws", 5: "k_chain_mfma_edge",
                6: "k_chain_mfma_ab", 7: "k_chain_fft1k", 8: "k_chain_decim_multi", 9: "k_chain_cos1k", 10: "k_chain_decim_w", 11: "k_chain_decim_b"}


class HipStep:
    """One rank's shard of the C2 workload through the C-ABI chain (dd_chain_*): the product path."""

    def __init__(self, args, rank, local_rank):
        import torch
        from directdemod_amd import _hip
        self.torch, self._hip = torch, _hip
        if not torch.cuda.is_available():
            raise SystemExit("bench.py needs an MI355X; no GPU visible")
        torch.cuda.set_device(local_rank)
        self.device = torch.device("cuda", local_rank)
        _hip.require_gpu()
        self.lib = lib = _hip.lib()
        _hip.check(lib.dd_set_device(local_rank), "dd_set_device")
        self.n = n = 1 << args.log2n
        halo = 256                         # >= ntaps-1+decim (255) and a multiple of 2 samples: keeps the shard 16-byte aligned
        self.start = rank * n              # absolute index of this rank's first sample
        self.pre = pre = halo if rank > 0 else 0
        self.xin = make_input(torch, n + pre, self.start - pre, self.device, 1235 + rank)
        self.out = torch.zeros(n + pre + 1, dtype=torch.float32, device=self.device)
        self.first = max(0, pre - 1)       # index of the shard's first output in `out` (ranks > 0: after the lead-in's)
        torch.cuda.synchronize()
        taps = np.ascontiguousarray(0.54 - 0.46 * np.cos(2.0 * np.pi * np.arange(NTAPS) / (NTAPS - 1)))
        flags = _hip.DD_CHAIN_NCO | _hip.DD_CHAIN_FM | (_hip.DD_CHAIN_FORCE_DIRECT if args.force_direct else 0)
        self.h = C.c_void_p()
        _hip.check(lib.dd_chain_create(C.byref(self.h), taps.ctypes.data_as(C.POINTER(C.c_double)), NTAPS,
                                       _hip.cycles_q64(F_OFFSET, FS), 1, flags), "dd_chain_create")
        self.stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        self.n_out = C.c_int64(0)

    def step(self):
        # new stream position, state derived from the absolute index alone.  Rank 0: the stream start
        # (history of ones).  Rank r: its shard plus the 256-sample lead-in in front of it as one chunk
        # from a zero history -- the lead-in's outputs (the first pre-1, with the filter still filling)
        # are not part of the shard; out[pre-1 : pre-1+n] is what rank r contributes (SURVEY.md 8e:
        # the halo is re-filtered locally, no exchange, no collective).  One launch per step on every rank.
        hip, lib = self._hip, self.lib
        hip.check(lib.dd_chain_seek(self.h, self.start - self.pre, self.stream), "dd_chain_seek")
        hip.check(lib.dd_chain_process(self.h, self.xin.data_ptr(), self.out.data_ptr(), self.n + self.pre,
                                       C.byref(self.n_out), self.stream), "dd_chain_process")

    def sync(self):
        self.torch.cuda.synchronize()

    def events(self):
        return self.torch.cuda.Event(enable_timing=True), self.torch.cuda.Event(enable_timing=True)

    def shard_output(self):
        """(tensor view, count): this rank's decoded outputs (rank 0 of the stream has one fewer, quirk Q3)"""
        cnt = int(self.n_out.value) - self.first
        return self.out[self.first:self.first + self.n], cnt

    def path(self):
        if self.lib.dd_chain_last_kernel(self.h) == 9:
            return "running-sums-f32"
        if self.lib.dd_chain_last_kernel(self.h) == 7:
            return "fft-f32-overlap-save"
        return {0: "direct-f32", 1: "mfma-f16x3"}.get(self.lib.dd_chain_path(self.h), str(self.lib.dd_chain_path(self.h)))

    def kernel(self):
        """the kernel the last step launched (one launch per step)"""
        return KERNEL_NAMES.get(self.lib.dd_chain_last_kernel(self.h), "?")

    def close(self):
        self.lib.dd_chain_destroy(self.h)


class StubStep:
    """DD_BENCH_STUB=1 (tests/test_bench_launcher.py): exercises the launcher, the rank set-up, the
    barriers, the max-over-ranks reduction and the gather leg on CPU with the gloo backend.  It computes
    nothing and its JSON line says so (`data: "stub"`); it is never a measurement."""

    class _Ev:
        def record(self):
            self.t = time.perf_counter()

        def elapsed_time(self, other):
            return (other.t - self.t) * 1e3

    def __init__(self, args, rank, local_rank):
        import torch
        self.torch = torch
        self.device = torch.device("cpu")
        self.n = 1 << min(args.log2n, 12)
        self.first = 0 if rank == 0 else 255
        self.rank = rank
        self.out = torch.full((self.n + 257,), float(rank), dtype=torch.float32)

    def step(self):
        time.sleep(0.0005)

    def sync(self):
        pass

    def events(self):
        return StubStep._Ev(), StubStep._Ev()

    def shard_output(self):
        return self.out[self.first:self.first + self.n], self.n - (1 if self.rank == 0 else 0)

    def path(self):
        return "stub"

    def kernel(self):
        return "stub"

    def close(self):
        pass


# ----------------------------------------------------------------------------- side configs (N = 1 only)
def side_roofline(key, alg_bytes, ms, bound="hbm", note=None):
    """The roofline block of a side entry: algorithmic bytes per launch / the measured time against the 8 TB/s HBM peak, with the HBM traffic
    of the same launch from profiles/hbm_traffic.json (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE in separate passes, tools/pmc_decimw_traffic.sh;
    not measured in this run) where a record exists."""
    achieved = alg_bytes / (ms * 1e-3) / 1e9
    r = {"bound": bound, "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 4),
         "traffic": None, "algorithmic_bytes_per_launch": int(alg_bytes), "basis": "HIP events around the timed launches"}
    try:
        rec = json.load(open(os.path.join(ROOT, "profiles", "hbm_traffic.json"))).get("kernels", {}).get(key)
        if rec:
            r["traffic"] = rec.get("bytes_per_launch_log2n_26")
            r["traffic_source"] = "profiles/hbm_traffic.json, %s at git %s" % (rec.get("kernel", key), rec.get("git", "?"))
    except Exception:
        pass
    if note:
        r["note"] = note
    return r


def side_configs(eng, steps=10, only_decim=False):
    """C3 / C4 front ends on the same device-resident buffer: the decimating fused chain,
    chunked with carried state as the reference's chunk loops do (decode_fm.py:54-70, decode_noaa.py:614-624).
    Reported in extra.side, never in `value`."""
    import scipy.signal as ss
    hip, lib = eng._hip, eng.lib
    n = eng.n
    k = np.arange(151)
    bh = 0.35875 - 0.48829 * np.cos(2 * np.pi * k / 150) + 0.14128 * np.cos(4 * np.pi * k / 150) - 0.01168 * np.cos(6 * np.pi * k / 150)
    rz = ss.remez(127, [0, 100e3, 150e3, 4999999], [1, 0], fs=1e7)
    res = []
    for name, taps, M, fs, f, chunk in (
            ("C3 front end: offsetFreq 250 kHz + remez127 + bwLim /50 + FM, 2^26 samples @10 MS/s in 16 chunks of 2^22", rz, 50, 10000000, 250000.0, 1 << 22),
            ("C4 front end: offsetFreq 30 kHz + blackmanHarris151 + bwLim /34 + FM, 2^26 samples @2.048 MS/s in chunks of 2e7", bh, 34, 2048000, 30000.0, 20000000)):
        taps = np.ascontiguousarray(taps, dtype=np.float64)
        h = C.c_void_p()
        hip.check(lib.dd_chain_create(C.byref(h), taps.ctypes.data_as(C.POINTER(C.c_double)), len(taps),
                                      hip.cycles_q64(f, fs), M, hip.DD_CHAIN_NCO | hip.DD_CHAIN_FM), "dd_chain_create")
        got = C.c_int64(0)
        bounds = [(a, min(n, a + chunk)) for a in range(0, n, chunk)]
        xin, out = eng.xin, eng.out

        def one_pass():
            hip.check(lib.dd_chain_reset(h, eng.stream), "dd_chain_reset")
            o = 0
            for a, b in bounds:
                hip.check(lib.dd_chain_process(h, xin.data_ptr() + 8 * a, out.data_ptr() + 4 * o, b - a, C.byref(got), eng.stream),
                          "dd_chain_process")
                o += got.value
            return o
        cb = (C.c_int64 * (len(bounds) + 1))(*([a for a, _ in bounds] + [n]))
        cn = (C.c_int64 * len(bounds))()

        def one_pass_chunk_list():
            # the same chunk list in ONE call (dd_chain_process_chunks: one launch, outputs bit-identical to the loop's)
            hip.check(lib.dd_chain_reset(h, eng.stream), "dd_chain_reset")
            hip.check(lib.dd_chain_process_chunks(h, xin.data_ptr(), out.data_ptr(), cb, len(bounds), cn, eng.stream), "dd_chain_process_chunks")
            return int(sum(cn))
        def timed(fn):
            for _ in range(3):
                r = fn()
            eng.sync()
            e0, e1 = eng.events()
            e0.record()
            for _ in range(steps):
                fn()
            e1.record()
            eng.sync()
            return e0.elapsed_time(e1) / steps, r
        ms_loop, n_out = timed(one_pass)
        ms, n_out_list = timed(one_pass_chunk_list)
        kern = KERNEL_NAMES.get(lib.dd_chain_last_kernel(h), "?")
        assert n_out_list == n_out
        # the same 2^26 samples as ONE chunk (one launch): what the kernel does without any chunk seam
        chunked_bounds = bounds
        bounds = [(0, n)]
        ms1, n_out1 = timed(one_pass)
        bounds = chunked_bounds
        assert n_out1 == n_out
        bps = 8.0 + 4.0 / M
        case = "C3" if M == 50 else "C4"
        alg = 8.0 * n + 4.0 * n_out
        u8 = None
        if case == "C4":
            # the same front end from RAW u8 pairs (what source.IQwav holds: 2 B per sample resident), one chunk
            import torch
            x8 = (xin[:n] + 127.5).round().clamp(0, 255).to(torch.uint8).contiguous()
            h8 = C.c_void_p()
            hip.check(lib.dd_chain_create(C.byref(h8), taps.ctypes.data_as(C.POINTER(C.c_double)), len(taps), hip.cycles_q64(f, fs), M,
                                          hip.DD_CHAIN_NCO | hip.DD_CHAIN_FM | hip.DD_CHAIN_U8_INPUT), "dd_chain_create")

            def one_pass_u8():
                hip.check(lib.dd_chain_reset(h8, eng.stream), "dd_chain_reset")
                hip.check(lib.dd_chain_process(h8, x8.data_ptr(), out.data_ptr(), n, C.byref(got), eng.stream), "dd_chain_process")
                return got.value
            ms8, n8 = timed(one_pass_u8)
            assert n8 == n_out
            u8 = {"ms": round(ms8, 4), "GS_per_s": round(n / ms8 / 1e6, 1), "bytes_per_sample": round(2.0 + 4.0 / M, 3),
                  "kernel": KERNEL_NAMES.get(lib.dd_chain_last_kernel(h8), "?"),
                  "roofline": side_roofline("k_chain_decim_b:C4u8", 2.0 * n + 4.0 * n_out, ms8, bound="issue",
                                            note="a quarter of the bytes: not memory bound -- the wave's own instruction stream (rotation and staging of a row, its "
                                                 "block sums on the matrix pipe, the discriminator) sets the time; the same launch WITHOUT its sample loads takes "
                                                 "the same time (profiles/r06_decimb_notes.txt)")}
            lib.dd_chain_destroy(h8)
            del x8
        res.append({"config": name, "chunks": len(bounds), "launches_per_pass": 1, "ms_per_pass": round(ms, 4), "outputs": n_out,
                    "roofline": side_roofline("k_chain_decim_b:" + case, alg, ms,
                                              note="reads every sample once, writes one angle per %d samples; what separates it from the peak: profiles/r06_decimb_notes.txt" % M),
                    "raw_u8_one_chunk": u8,
                    "GS_per_s": round(n / ms / 1e6, 1), "bytes_per_sample": round(bps, 3),
                    "frac_of_8TBs": round(n * bps / (ms * 1e-3) / 8e12, 4),
                    "kernel": kern,
                    "how": "dd_chain_process_chunks: the whole chunk list in one launch (k_chain_decim_b: the list is one chunk on the absolute sample grid)",
                    "chunk_loop": {"launches_per_pass": len(bounds), "ms": round(ms_loop, 4), "GS_per_s": round(n / ms_loop / 1e6, 1),
                                   "frac_of_8TBs": round(n * bps / (ms_loop * 1e-3) / 8e12, 4)},
                    "one_chunk": {"ms": round(ms1, 4), "GS_per_s": round(n / ms1 / 1e6, 1),
                                  "frac_of_8TBs": round(n * bps / (ms1 * 1e-3) / 8e12, 4),
                                  "roofline": side_roofline("k_chain_decim_b:" + case, alg, ms1)}})
        lib.dd_chain_destroy(h)
    if only_decim:                                            # (tools/bench_decim.py)
        return res
    # the headline chain on RAW u8 input (what source.IQwav reads: 2 B/sample resident instead of 8) and with complex64
    # output (commSignal.filter without demod_fm), same kernel family
    import torch
    ham = np.ascontiguousarray(0.54 - 0.46 * np.cos(2.0 * np.pi * np.arange(NTAPS) / (NTAPS - 1)))
    x8 = (eng.xin[:n] + 127.5).round().clamp(0, 255).to(torch.uint8).contiguous()
    for name, flags, src, esz, bps in (
            ("C2 chain on raw u8 input (source.py:117-118 widened on the device), FM out", hip.DD_CHAIN_NCO | hip.DD_CHAIN_FM | hip.DD_CHAIN_U8_INPUT, x8, 2, 6.0),
            ("C2 front end with complex64 output (offsetFreq + Hamming 255, no demod)", hip.DD_CHAIN_NCO, eng.xin, 8, 16.0)):
        h = C.c_void_p()
        hip.check(lib.dd_chain_create(C.byref(h), ham.ctypes.data_as(C.POINTER(C.c_double)), NTAPS, hip.cycles_q64(F_OFFSET, FS), 1, flags),
                  "dd_chain_create")
        got = C.c_int64(0)
        out = torch.empty(2 * n, dtype=torch.float32, device=eng.out.device) if bps == 16.0 else eng.out

        def step():
            hip.check(lib.dd_chain_reset(h, eng.stream), "dd_chain_reset")
            hip.check(lib.dd_chain_process(h, src.data_ptr(), out.data_ptr(), n, C.byref(got), eng.stream), "dd_chain_process")
        for _ in range(100):
            step()
        eng.sync()
        e0, e1 = eng.events()
        e0.record()
        for _ in range(10 * steps):
            step()
        e1.record()
        eng.sync()
        ms = e0.elapsed_time(e1) / (10 * steps)
        kname = KERNEL_NAMES.get(lib.dd_chain_last_kernel(h), "?")
        entry = {"config": name + ", 2^26 samples, one chunk", "kernel": kname,
                 "ms_per_pass": round(ms, 4), "GS_per_s": round(n / ms / 1e6, 1),
                 "bytes_per_sample": bps, "frac_of_8TBs": round(n * bps / (ms * 1e-3) / 8e12, 4)}
        # which bound, from the records under profiles/ (not measured in this run)
        try:
            pw = json.load(open(os.path.join(ROOT, "profiles", "power.json"))).get("kernels", {}).get(kname + (":u8" if bps == 6.0 else ":cx"))
        except Exception:
            pw = None
        if bps == 6.0:
            entry["bound"] = {"name": "package power (and the arithmetic itself)", "power": pw,
                              "ms_floor_at_the_1400W_cap": pw.get("ms_floor_at_the_cap") if pw else None,
                              "ms_arithmetic_only": [0.0887, 0.0932],
                              "note": "6 B per sample: a third of the HBM rate the FM flavour needs, so memory does not bind; the running sums alone take 0.089-0.093 ms "
                                      "(tools/ubench/cosfir_arith.hip, profiles/r05_cosfir_ubench.txt) and the launch draws the board's cap: its dynamic energy over "
                                      "(1400 W - idle) is the floor quoted here (profiles/power.json) -- the measured time is within ~5 % of it"}
        else:
            entry["bound"] = {"name": "HBM, 1 : 1 read : write", "power": pw, "copy_ceiling_TBs": 5.61,
                              "frac_of_copy_ceiling": round(n * bps / (ms * 1e-3) / 5.61e12, 3),
                              "note": "16 B per sample (8 in, 8 out): a float4 copy kernel reaches 5.61 TB/s of read + written bytes on this part (profiles/r04_stream_2to1.txt, "
                                      "first rows; the guide: 6.29); the clock stays at its maximum and the package below the cap (profiles/power.json)"}
        res.append(entry)
        lib.dd_chain_destroy(h)
        del out
    # SURVEY 8(d) defines two C2 inputs: B (FM tone + noise, the headline above) and A, what source.py:117-118 hands out on a dead
    # channel -- I, Q iid uniform integers 0..255 minus 127.5, np.random.default_rng(1234).  The angle stage is data dependent
    # (a group of 256 outputs takes the small-angle arctangent only if every |angle| in it is below 22.5 degrees), so both are
    # timed here through the same call, the same way, back to back.
    xa = (torch.from_numpy(np.random.default_rng(1234).integers(0, 256, size=(n, 2), dtype=np.uint8)).to(eng.out.device).float() - 127.5).contiguous()
    h = C.c_void_p()
    hip.check(lib.dd_chain_create(C.byref(h), ham.ctypes.data_as(C.POINTER(C.c_double)), NTAPS, hip.cycles_q64(F_OFFSET, FS), 1,
                                  hip.DD_CHAIN_NCO | hip.DD_CHAIN_FM), "dd_chain_create")
    got = C.c_int64(0)
    ab = {}
    for rnd in range(2):
        for name, src in (("B", eng.xin), ("A", xa)):
            def step():
                hip.check(lib.dd_chain_reset(h, eng.stream), "dd_chain_reset")
                hip.check(lib.dd_chain_process(h, src.data_ptr(), eng.out.data_ptr(), n, C.byref(got), eng.stream), "dd_chain_process")
            for _ in range(100):
                step()
            eng.sync()
            e0, e1 = eng.events()
            e0.record()
            for _ in range(10 * steps):
                step()
            e1.record()
            eng.sync()
            ab[name] = min(ab.get(name, 1e9), e0.elapsed_time(e1) / (10 * steps))
    kname = KERNEL_NAMES.get(lib.dd_chain_last_kernel(h), "?")
    lib.dd_chain_destroy(h)
    del xa
    res.append({"config": "C2 input A (I, Q iid uniform u8 noise, default_rng(1234): SURVEY 8d; source.py:117-118) beside input B (the headline's FM tone + noise), same call, back to back, 2^26 samples",
                "kernel": kname, "ms_per_pass_input_A": round(ab["A"], 4), "ms_per_pass_input_B": round(ab["B"], 4),
                "input_A_over_B": round(ab["A"] / ab["B"], 4), "bytes_per_sample": 12.0,
                "frac_of_8TBs_input_A": round(n * 12.0 / (ab["A"] * 1e-3) / 8e12, 4), "frac_of_8TBs_input_B": round(n * 12.0 / (ab["B"] * 1e-3) / 8e12, 4)})
    res.append(side_headline_kernels(eng, steps))
    try:
        res.append(side_iir_iq(eng))
    except Exception as e:
        res.append({"config": "butter at IQ rate", "error": repr(e)})
    res.append(side_c3_end_to_end(eng, steps))
    res.append(side_c3_through_classes(eng, steps))
    res.extend(side_c4_end_to_end())
    res.append(side_ring_feeder())
    return res


def side_iir_iq(eng, steps=5):
    """filters.butter over full-rate IQ (decode_funcube.py:160,230: the Funcube / Meteor front ends low-pass the complex stream before they
    decimate): a 6th-order Butterworth low-pass, butter(2 048 000, 20 000), over the 2^26 resident complex64 samples through the drop-in class
    -- complex128 out like the reference's lfilter (csrc/dd_fir.hip: block end states, scan of the block start states, blocks
    re-run from their true states)."""
    from directdemod_amd import _hip, filters
    import torch
    n = eng.n
    f = filters.butter(2048000, 20000.0, storeState=False)
    src = _hip.DevArray(n, np.complex64, ptr=eng.xin.data_ptr())      # (a view of the bench's resident input: nothing is copied)
    # (the 1 GiB output was the buffer pool's whole budget until round 6 -- with anything else parked there it was hipMalloc'ed and hipFree'd on
    #  every pass, 30 ms of allocator in one record; the budget is 16 GiB now, the pool is still emptied first and one output alive at a time)
    _hip.pool_trim(0)
    y = f.applyOn(src)
    _hip.sync()
    del y
    t0 = time.perf_counter()
    for _ in range(steps):
        y = f.applyOn(src)
        del y
    _hip.sync()
    ms = (time.perf_counter() - t0) / steps * 1e3
    y = None
    alg = 24.0 * n                                            # 8 B read (complex64) + 16 B written (complex128) per sample
    del y
    return {"config": "filters.butter(2 048 000, 20 000), order 6, over 2^26 complex64 IQ samples (decode_funcube.py:160 shape), complex128 out, through the class",
            "ms_per_pass": round(ms, 3), "GS_per_s": round(n / ms / 1e6, 2), "bytes_per_sample": 24.0,
            "roofline": side_roofline("dd_iir_c64:iq", alg, ms, note="float64 recurrence in three passes over the samples (block end states from zero, the scan of "
                                      "the block start states, the blocks again from their true states); round 6: the passes read the complex64 samples as they are "
                                      "(dd_iir_c64: 8 + 8 + 16 = 32 B per sample move, 1.33 x the algorithmic bytes; 72 through the widened copy before), in 256-byte "
                                      "pieces per block and step -- 65 536 sequential streams, ~3 TB/s; wall clock around the class calls, host side included")}


def side_headline_kernels(eng, steps=10):
    """The headline chain through each M = 1 kernel that takes Hamming 255 + FM, same call, back to back (dd_debug_select_kernel):
    k_chain_cos1k (running sums, the choice by tap class since round 5), k_chain_fft1k (overlap-save FFT, rounds 3-4),
    k_chain_mfma_ab (f16-limb Toeplitz on the matrix cores, round 2)."""
    hip, lib = eng._hip, eng.lib
    n = eng.n
    ham = np.ascontiguousarray(0.54 - 0.46 * np.cos(2.0 * np.pi * np.arange(NTAPS) / (NTAPS - 1)))
    before = os.environ.get("DD_MFMA_KERNEL")
    out = {"config": "C2 headline through each M = 1 kernel, same call, 2^26 samples", "bytes_per_sample": 12.0, "kernels": {}}
    try:
        for sel in (None, "fft1k", "ab"):
            hip.select_kernel(sel)
            h = C.c_void_p()
            hip.check(lib.dd_chain_create(C.byref(h), ham.ctypes.data_as(C.POINTER(C.c_double)), NTAPS, hip.cycles_q64(F_OFFSET, FS), 1,
                                          hip.DD_CHAIN_NCO | hip.DD_CHAIN_FM), "dd_chain_create")
            got = C.c_int64(0)

            def step():
                hip.check(lib.dd_chain_reset(h, eng.stream), "dd_chain_reset")
                hip.check(lib.dd_chain_process(h, eng.xin.data_ptr(), eng.out.data_ptr(), n, C.byref(got), eng.stream), "dd_chain_process")
            for _ in range(300):
                step()
            eng.sync()
            e0, e1 = eng.events()
            e0.record()
            for _ in range(20 * steps):
                step()
            e1.record()
            eng.sync()
            ms = e0.elapsed_time(e1) / (20 * steps)
            out["kernels"][KERNEL_NAMES.get(lib.dd_chain_last_kernel(h), "?")] = {
                "ms_per_pass": round(ms, 4), "GS_per_s": round(n / ms / 1e6, 1), "frac_of_8TBs": round(n * 12.0 / (ms * 1e-3) / 8e12, 4)}
            lib.dd_chain_destroy(h)
    finally:
        hip.select_kernel(before)
    return out


def side_ring_feeder(log2n=28):
    """source.IQwav-style ingest (source.py:95-118, BASELINE north_star: pinned-host ring buffers, hipMemcpyAsync on a side stream):
    a host-resident u8 recording through stream.stream_fm_chain -- raw pairs over PCIe into device slots on a copy stream while the
    previous chunk is decoded (C4 front end: offsetFreq 30 kHz + blackmanHarris151 + bwLim /34 + FM).  Wall time, PCIe inclusive:
    never `value`."""
    from directdemod_amd import source, stream as st
    nraw = 1 << log2n
    raw = np.random.default_rng(1).integers(0, 256, size=(nraw, 2), dtype=np.uint8)
    src = source.IQarray(raw, 2048000)
    k = np.arange(151)
    bh = 0.35875 - 0.48829 * np.cos(2 * np.pi * k / 150) + 0.14128 * np.cos(4 * np.pi * k / 150) - 0.01168 * np.cos(6 * np.pi * k / 150)
    st.stream_fm_chain(src, bh, 30000.0, 34, chunk_size=20000000)
    best = None
    for _ in range(3):
        t0 = time.perf_counter()
        st.stream_fm_chain(src, bh, 30000.0, 34, chunk_size=20000000, staging="direct")
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    gbps = 2.0 * nraw / best / 1e9
    return {"config": "ring feeder: host-resident u8 recording over PCIe (hipMemcpyAsync on a copy stream, chunks of 2e7 samples) through "
                      "the C4 front end (BH151 /34 FM), 2^%d samples" % log2n,
            "s_per_pass_wall": round(best, 4), "GS_per_s": round(nraw / best / 1e9, 2), "host_to_device_GBps": round(gbps, 1),
            "frac_of_pcie_63GBps": round(gbps / 63.0, 3), "staging": "direct (from the recording's own memory)"}


# ----------------------------------------------------------------------------- one rank
def side_c3_end_to_end(eng, steps=10):
    """config 3 end to end (decode_fm.py:54-70): 2^26 samples @10 MS/s in sixteen chunks of 2^22, each chunk offsetFreq
    250 kHz + remez127 + bwLim /50 + FM (state carried) and then bwLim(11025, strict) = scipy.signal.resample of ITS outputs
    (comm.py:110-116: 83886 or 83887 samples -> 4624).  Two calls: dd_chain_process_chunks (one launch) and
    dd_resample_fft_chunks (one chirp-z batch: these lengths have large prime factors)."""
    import scipy.signal as ss
    import torch
    hip, lib = eng._hip, eng.lib
    n, chunk, M, fs, f = eng.n, 1 << 22, 50, 10000000, 250000.0
    rz = np.ascontiguousarray(ss.remez(127, [0, 100e3, 150e3, 4999999], [1, 0], fs=1e7), dtype=np.float64)
    h = C.c_void_p()
    hip.check(lib.dd_chain_create(C.byref(h), rz.ctypes.data_as(C.POINTER(C.c_double)), len(rz), hip.cycles_q64(f, fs), M,
                                  hip.DD_CHAIN_NCO | hip.DD_CHAIN_FM), "dd_chain_create")
    nch = n // chunk
    cb = (C.c_int64 * (nch + 1))(*[i * chunk for i in range(nch + 1)])
    cn = (C.c_int64 * nch)()
    audio = torch.empty(nch * 4700, dtype=torch.float64, device=eng.out.device)
    A = C.c_int64 * nch
    state = {}

    def one_pass():
        hip.check(lib.dd_chain_reset(h, eng.stream), "dd_chain_reset")
        hip.check(lib.dd_chain_process_chunks(h, eng.xin.data_ptr(), eng.out.data_ptr(), cb, nch, cn, eng.stream), "dd_chain_process_chunks")
        lens = list(cn)
        if "args" not in state:                      # chunk lengths are host arithmetic: the same every pass
            nums = [int(11025 * v / (fs // M)) for v in lens]
            ioff = [sum(lens[:i]) for i in range(nch)]
            ooff = [sum(nums[:i]) for i in range(nch)]
            state["args"] = (A(*ioff), A(*lens), A(*ooff), A(*nums), sum(nums), sorted(set(lens)))
        ioff, ln, ooff, nm, tot, _ = state["args"]
        hip.check(lib.dd_resample_fft_chunks(eng.out.data_ptr(), 1, ioff, ln, audio.data_ptr(), ooff, nm, nch, eng.stream), "dd_resample_fft_chunks")
        return tot
    for _ in range(3):
        tot = one_pass()
    eng.sync()
    e0, e1 = eng.events()
    e0.record()
    for _ in range(steps):
        one_pass()
    e1.record()
    eng.sync()
    ms = e0.elapsed_time(e1) / steps
    lib.dd_chain_destroy(h)
    return {"config": "C3 end to end (front end + FFT resample to 11 025 S/s), 2^26 samples @10 MS/s in 16 chunks of 2^22",
            "ms_per_pass": round(ms, 4), "GS_per_s": round(n / ms / 1e6, 1), "audio_samples": int(tot), "chunk_output_lengths": state["args"][5],
            "how": "dd_chain_process_chunks + dd_resample_fft_chunks: 1 chain launch; the 16 resamples as ONE chirp-z batch for the 2313 bins kept (3.2^15-point convolutions, chunk lengths mixed)"}


def side_c3_through_classes(eng, steps=10):
    """The same C3 job written as the reference writes it (decode_fm.py:54-70) against the drop-in classes -- chunker,
    commSignal(...).offsetFreq.filter.bwLim.funcApply(fm.demod).bwLim(strict), extend -- on slices of the device-resident
    input.  Wall clock per pass (the Python of sixteen chunks included), the result read on the device at the end."""
    import time
    import scipy.signal as ss
    from directdemod_amd import comm, filters, demod_fm, chunker, _hip
    n, chunk, fs = eng.n, 1 << 22, 10000000
    res = _hip.DevArray(n, np.complex64, ptr=eng.xin.data_ptr(), base=eng.xin)
    taps = np.ascontiguousarray(ss.remez(127, [0, 100e3, 150e3, 4999999], [1, 0], fs=1e7))
    objs = {}

    class _Src:
        length = n

    def one_pass(fresh):
        if fresh or not objs:
            objs["rz"], objs["fm"] = filters.filter(taps, 1, storeState=True), demod_fm.demod_fm()
        rz, fm = objs["rz"], objs["fm"]
        ck = chunker.chunker(_Src(), chunk)
        out = comm.commSignal(11025)
        for a, b in ck.getChunks:
            out.extend(comm.commSignal(fs, res.view(a, b - a), ck).offsetFreq(250000.0).filter(rz)
                       .bwLim(200000, uniq="First").funcApply(fm.demod).bwLim(11025, True))
        return out.length, out.device_signal

    def timed(fresh):
        for _ in range(3):
            tot, _d = one_pass(fresh)
        _hip.sync()
        t0 = time.perf_counter()
        for _ in range(steps):
            tot, _d = one_pass(fresh)
        _hip.sync()
        return (time.perf_counter() - t0) * 1e3 / steps, tot
    ms_fresh, tot = timed(True)
    ms, _ = timed(False)
    rz = objs["rz"]
    return {"config": "C3 end to end through the drop-in classes (chunker / commSignal / filter / demod_fm, 16 chunks of 2^22, device-resident input)",
            "ms_per_pass_wall": round(ms, 4), "ms_per_pass_wall_new_filter_and_demod_objects_each_pass": round(ms_fresh, 4),
            "GS_per_s": round(n / ms / 1e6, 1), "audio_samples": int(tot), "kernel": KERNEL_NAMES.get(rz._last_kernel(), "?"), "how": "recorded chunk loop -> dd_fused_process_chunks + dd_resample_fft_chunks when the output is read"}


def synth_apt_iq(duration_s, fs=2048000, seed=1, f_offset=30000.0, dev=17000.0, amp=60.0, sigma=4.0):
    """The C4 workload: synthetic NOAA-APT-shaped IQ on the u8 grid -- 2 lines/s x 2080 words at 4160 words/s,
    sync A at words 0-39 and sync B at 1040-1079 mapped (bit*233+11)/255, AM on a 2400 Hz subcarrier, FM (dev Hz) at
    +f_offset, amplitude 60 + complex noise sigma 4.  The same generator as the test suite's (tests/test_host_logic.py
    checks the two produce identical bytes), kept here so that the bench imports nothing from oracle/ outside its
    cpu_baseline leg."""
    from directdemod_amd import constants
    sync_a, sync_b = np.asarray(constants.NOAA_SYNCA), np.asarray(constants.NOAA_SYNCB)
    rng = np.random.default_rng(seed)
    n = int(duration_s * fs)
    nwords = int(math.ceil(duration_s * 4160)) + 1
    words = rng.uniform(0.2, 0.8, size=nwords)
    for line_start in range(0, nwords, 2080):
        for k in range(40):
            if line_start + k < nwords:
                words[line_start + k] = (sync_a[k] * 233 + 11) / 255.0
            if line_start + 1040 + k < nwords:
                words[line_start + 1040 + k] = (sync_b[k] * 233 + 11) / 255.0
    out = np.empty((n, 2), dtype=np.uint8)
    blk = 1 << 20
    phase = 0.0
    for s0 in range(0, n, blk):
        s1 = min(n, s0 + blk)
        idx = np.arange(s0, s1)
        t = idx / fs
        env = words[np.minimum((idx * 4160) // fs, nwords - 1)]
        audio = env * np.sin(2 * np.pi * 2400.0 * t)
        ph = phase + 2 * np.pi * dev * np.cumsum(audio) / fs
        phase = ph[-1]
        s = amp * np.exp(1j * (2 * np.pi * f_offset * t + ph))
        s = s + sigma * (rng.standard_normal(s1 - s0) + 1j * rng.standard_normal(s1 - s0))
        out[s0:s1, 0] = np.clip(np.round(s.real + 127.5), 0, 255).astype(np.uint8)
        out[s0:s1, 1] = np.clip(np.round(s.imag + 127.5), 0, 255).astype(np.uint8)
    return out


def side_c4_end_to_end(dur=60.0):
    """config 4 end to end at bench duration: getCrudeSync + getAccurateSync (decode_noaa.py:769-880) over a
    60 s synthetic APT recording resident in HBM as raw u8 pairs; its index lists are the ones tests/test_gpu_audio.py
    compares with the reference's own run (tests/golden/noaa_c4_60s.npz).  Wall time of the two calls, host logic included."""
    from directdemod_amd import noaa_sync, source, _hip
    raw = synth_apt_iq(dur, 2048000, seed=1)
    src = source.IQarray(raw, 2048000)

    def one():
        obj = noaa_sync.noaa_sync(src, 30000.0)
        _hip.sync()
        t0 = time.perf_counter()
        sa, sb = obj.getCrudeSync()
        _hip.sync()
        t1 = time.perf_counter()
        acc = obj.getAccurateSync()
        _hip.sync()
        t2 = time.perf_counter()
        return (t1 - t0) * 1e3, (t2 - t1) * 1e3, len(sa), len(sb), len(acc[0][0]) + len(acc[1][0])
    one()                                   # plans, first launches, upload of the recording
    runs = [one() for _ in range(3)]
    crude = min(r[0] for r in runs)
    accurate = min(r[1] for r in runs)
    warm = {"config": "C4 end to end 60 s (crude + accurate sync), 2.048 MS/s synthetic APT, recording resident in HBM as u8",
            "iq_samples": int(src.length), "crude_sync_ms": round(crude, 3), "accurate_sync_ms": round(accurate, 3),
            "total_ms": round(crude + accurate, 3), "syncs": [runs[0][2], runs[0][3]], "accurate_windows": runs[0][4],
            "GS_per_s": round(src.length / (crude + accurate) / 1e6, 2)}
    # what bounds the two calls.  Not measured in this run: byte counts per kernel from profiles/r04_side_traffic.txt (PMC), arithmetic
    # from the stage definitions, launches from profiles/r05_bench_kernel_stats.csv.
    nwin = runs[0][4]
    hbm_mb_per_win = 24.3        # fetched + written by the nine kernels of a batch / windows of the batch (1452 MB per 59.75 windows)
    f32_mflop_per_win = 288.0    # the zero-phase blackmanHarris(151) pre-filter at IQ rate: 2 passes x (118 152 + 6 x 151) samples x 151 taps x 8 flop
    f64_mflop_per_win = 60.0     # Hilbert envelope as one 2^18-point float64 cyclic convolution (2 transforms x 5 N log2 N) + Hamming-492 filtfilt (cosine form) + prefix sums
    t_hbm = nwin * hbm_mb_per_win * 1e6 / 8e12 * 1e3
    t_f32 = nwin * f32_mflop_per_win * 1e6 / 157.3e12 * 1e3
    t_f64 = nwin * f64_mflop_per_win * 1e6 / 78.6e12 * 1e3     # (78.6 TF: AMD's public FP64 vector figure for MI355X; MI355X_MICROARCH.md lists none)
    t_mix = t_f32 + t_hbm * (1.0 - 190.0 / 1452.0)            # the two pre-filter passes are arithmetic bound, the other seven kernels memory bound
    warm["bound"] = {
        "accurate_sync": {"windows": nwin, "launches": 9 * ((runs[0][2] + 63) // 64 + (runs[0][3] + 63) // 64),
                          "hbm_bytes": int(nwin * hbm_mb_per_win * 1e6), "f32_flop": int(nwin * f32_mflop_per_win * 1e6), "f64_flop": int(nwin * f64_mflop_per_win * 1e6),
                          "ms_at_8TBs": round(t_hbm, 3), "ms_at_157TF_f32": round(t_f32, 3), "ms_at_78.6TF_f64": round(t_f64, 3),
                          "ms_sum_of_per_kernel_bounds": round(t_mix, 3), "measured_over_bound": round(accurate / t_mix, 2)},
        "crude_sync": {"front_end_ms_alone": 0.066, "note": "the decimating front end from raw u8 (k_chain_decim_b, issue bound: extra.side C4 raw_u8_one_chunk) is a "
                       "tenth of the call; the rest is ~25 float64 launches of 5-50 us over 3.6 M audio samples (envelope in 240 000-sample blocks, two "
                       "normalised correlations, radix select, candidate scan) and one host synchronisation: launch- and latency-bound at ~2 us per "
                       "dependent kernel boundary (MI355X_MICROARCH.md, price list 'boundary'), no byte or flop bound within a factor of five"},
        "source": "profiles/r04_side_traffic.txt (bytes per kernel, PMC), profiles/r05_bench_kernel_stats.csv (launches), DESIGN.md 4.5; not measured in this run"}
    # the reference decodes one file per process (main.py:208-270): the FIRST call of a fresh process is the call.  A child process
    # (started, never exec'ed into) loads the same recording from a scratch file and times its first crude + accurate sync.
    cold = {"config": "C4 end to end 60 s, FIRST call of a fresh process (recording on the host: upload, code objects, tables and plans included)"}
    import subprocess
    import tempfile
    path = None
    try:
        fd, path = tempfile.mkstemp(suffix=".npy", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
        os.close(fd)
        np.save(path, raw)
        # (host-side time stamps inside the library's calls, to stderr: kept in the entry so that a slow first call says where it went)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_noaa_cold.py"), path], capture_output=True, text=True, timeout=300,
                           env=dict(os.environ, DD_CRUDE_TRACE="1", DD_SYNC_TRACE="1"))
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        if r.returncode == 0 and line:
            cold.update(json.loads(line[-1]))
            cold["host_time_stamps"] = [ln.strip() for ln in r.stderr.splitlines() if " host us" in ln][:8]
        else:
            cold["error"] = (r.stderr or r.stdout)[-400:]
    except Exception as e:
        cold["error"] = repr(e)
    finally:
        if path and os.path.exists(path):
            os.unlink(path)
    return [warm, cold]


# ----------------------------------------------------------------------------- --dump-outputs
DUMP_EDGE = 1 << 16            # outputs kept whole at each end of the shard (the stream start / end and their edge tiles)
DUMP_SAMPLE = 1 << 21          # seeded sample positions per GPU in between: 8 MB of float32 angles + 16 MB of float64 positions
DUMP_SEED = 20261016


def dump_outputs(eng, path, rank, world):
    """--dump-outputs: this rank's decoded angles as the last timed step left them (float32 radians, the count the call returned).
    Files, prefixed rank<r>_ with more than one rank: fm_angle_head / fm_angle_tail (the first / last DUMP_EDGE outputs),
    fm_angle_sample + fm_angle_sample_index (the outputs at sorted positions drawn from a fixed seed, DUMP_SAMPLE per GPU shared
    among the ranks; every output when there are no more than that), fm_angle_count.  24 MB + 0.5 MB per rank in all."""
    torch = eng.torch
    out, cnt = eng.shard_output()
    out = out[:cnt]
    k = max(1, DUMP_SAMPLE // world)
    if cnt <= k:
        idx = np.arange(cnt, dtype=np.int64)
    else:
        idx = np.unique(np.random.default_rng(DUMP_SEED + rank).integers(0, cnt, size=k, dtype=np.int64))
    arrays = {
        "fm_angle_head": out[:DUMP_EDGE],
        "fm_angle_tail": out[max(0, cnt - DUMP_EDGE):],
        "fm_angle_sample": out[torch.from_numpy(idx).to(out.device)],
    }
    os.makedirs(path, exist_ok=True)
    pre = "rank%d_" % rank if world > 1 else ""
    for name, t in arrays.items():
        np.save(os.path.join(path, pre + name + ".npy"), t.detach().cpu().numpy().astype(np.float32))
    np.save(os.path.join(path, pre + "fm_angle_sample_index.npy"), idx.astype(np.float64))
    np.save(os.path.join(path, pre + "fm_angle_count.npy"), np.array([cnt], dtype=np.float64))


def run_rank(args):
    import torch
    import torch.distributed as dist

    stub = bool(os.environ.get("DD_BENCH_STUB"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    # DD_BENCH_ONE_DEVICE=1 (tests on a 1-GPU box): every rank computes on cuda:0 and the ranks talk over gloo -- the real
    # engine, the halo lead-in of ranks > 0, the barriers and the gather are exercised by N processes sharing one GPU.
    # Its line is marked `data: "synthetic (ranks share one GPU)"`; it is a functional check, not a scaling measurement.
    one_device = bool(os.environ.get("DD_BENCH_ONE_DEVICE"))
    if one_device:
        local_rank = 0
    if args.simulate_rank is not None:
        rank = args.simulate_rank
    if not stub and not one_device and world > 1 and torch.cuda.device_count() < world:
        # started directly under torch.distributed.run on a node with fewer GPUs than ranks (device_count() does not
        # initialise the GPU): one line from rank 0, every rank leaves with the same code
        if rank == 0:
            sys.stderr.write("bench.py: %d ranks, %d GPU(s) visible on this node\n" % (world, torch.cuda.device_count()))
        raise SystemExit(2)
    # DD_BENCH_FORCE_DIST=1 (tests/test_gpu_bench_nccl.py): take the distributed branch with ONE rank too -- process group on the
    # nccl (= RCCL) backend, barriers, the variable-count gather and the timed all_gather -- so that the RCCL leg has run on the
    # 1-GPU test box before the driver's 8-GPU node is the first place it ever executes
    dist_on = world > 1 or bool(os.environ.get("DD_BENCH_FORCE_DIST"))
    if not stub:
        build_once_per_node()                      # before any rendezvous: ranks never race on the build
    if dist_on:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
    eng = (StubStep if stub else HipStep)(args, rank, local_rank)
    device = eng.device
    cdev = torch.device("cpu") if one_device else device       # where the small reduction tensors live
    rccl_init_s = None
    if dist_on:
        # one node by contract: the bootstrap sockets stay on loopback (a container hostname may not resolve, and a probe of
        # every interface of a fresh box is the kind of wait a record cannot explain); the data path is xGMI / shared memory
        os.environ.setdefault("NCCL_SOCKET_IFNAME", "lo")
        os.environ.setdefault("GLOO_SOCKET_IFNAME", "lo")
        from datetime import timedelta
        t_init = time.perf_counter()
        if stub or one_device:
            dist.init_process_group("gloo", rank=rank, world_size=world, timeout=timedelta(seconds=300))
        else:
            # (300 s, not 60 -- a cold 8-GPU RCCL communicator build has never run here; how long it took is reported as
            #  extra.rccl_init_s, the expectation of well under a minute stays a number to read, not a reason to abort)
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=device, timeout=timedelta(seconds=300))
        t_pg = time.perf_counter()
        # the communicator itself is built lazily by the first collective: time that too, it is what an 8-GPU record shows first
        warm = torch.zeros(1, dtype=torch.float32, device=torch.device("cpu") if (stub or one_device) else device)
        dist.all_reduce(warm)
        if not (stub or one_device):
            torch.cuda.synchronize(device)
        rccl_init_s = time.perf_counter() - t_init
        sys.stderr.write("[bench] rank %d/%d: init_process_group %.2f s, first collective %.2f s\n" %
                         (rank, world, t_pg - t_init, rccl_init_s - (t_pg - t_init)))
        sys.stderr.flush()
    n = eng.n
    step = eng.step

    def barrier():
        eng.sync()
        if dist_on:
            dist.barrier()
        eng.sync()

    # --full: cold figures: the first step this process runs (one-off costs: code object load, the taps' spectrum, tables) and the
    # 19 steps after it, before any pre-roll (HIP events on the launch stream).  tools/debug/cold_steps.py shows the profile: launch 1
    # ~8 ms, launches 2-6 at the steady time, then 15-35 % slower for ~80 launches while the power controller settles
    first_ms = cold_ms = 0.0
    if args.full:
        cold_steps = 20
        f0, c0, c1 = eng.events() + (eng.events()[0],)
        f0.record()
        step()
        c0.record()
        for _ in range(cold_steps - 1):
            step()
        c1.record()
        eng.sync()
        first_ms = f0.elapsed_time(c0)
        cold_ms = c0.elapsed_time(c1) / (cold_steps - 1)

    ramp_steps = 0
    t_ramp = time.perf_counter()
    while (time.perf_counter() - t_ramp) * 1e3 < args.ramp_ms:          # untimed clock pre-roll
        for _ in range(25):
            step()
        eng.sync()
        ramp_steps += 25
    for _ in range(args.warmup):
        step()
    barrier()
    # the hot kernel's launch duration: HIP events on the launch stream around the K timed launches
    # (the chain is ONE kernel launch per step -- edge tiles ride along in it -- so elapsed / K is the
    # average launch duration, launch gaps included)
    ev0, ev1 = eng.events()
    t0 = time.perf_counter()
    ev0.record()
    for i in range(args.steps):
        step()
    ev1.record()
    barrier()
    dt = time.perf_counter() - t0
    kern_ms = ev0.elapsed_time(ev1) / args.steps
    if args.dump_outputs:
        dump_outputs(eng, args.dump_outputs, rank, world)

    # --full: the same step for >= --steady-ms of device time (20 steps are ~3 ms; the default 6 s also makes the run visible to an
    # activity sampler that looks every few seconds): consistency check of the short region
    long_steps, long_ms = 0, 0.0
    if args.full:
        long_steps = max(args.steps, int(np.ceil((min(args.steady_ms, 50.0) if stub else args.steady_ms) / max(kern_ms, 1e-3))))
        l0, l1 = eng.events()
        l0.record()
        for i in range(long_steps):
            step()
        l1.record()
        barrier()
        long_ms = l0.elapsed_time(l1) / long_steps

    tmax = torch.tensor([dt, kern_ms, long_ms, cold_ms, first_ms], dtype=torch.float64, device=cdev)
    per_rank = None
    if dist_on:
        allk = [torch.zeros_like(tmax) for _ in range(world)]
        dist.all_gather(allk, tmax)
        per_rank = [round(float(t[1]), 4) for t in allk]
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
    dt_max, kern_ms_max, long_ms_max, cold_ms_max, first_ms_max = (float(v) for v in tmax)

    extra = {}
    if dist_on:
        extra["backend"] = dist.get_backend()
        extra["world_size_seen"] = dist.get_world_size()
        ri = torch.tensor([rccl_init_s], dtype=torch.float64, device=cdev)
        dist.all_reduce(ri, op=dist.ReduceOp.MAX)
        extra["rccl_init_s"] = round(float(ri[0]), 3)          # rendezvous + process group + first collective, slowest rank
    if dist_on and args.full and not args.no_gather:
        from directdemod_amd import shard
        shard_out, cnt = eng.shard_output()                 # this rank's outputs (a view) and how many are valid
        if one_device:
            shard_out = shard_out.cpu()                     # gloo leg of the one-device functional check
        parts = shard.gather_outputs(shard_out, cnt, world, dist, force=True)      # variable counts: checks the assembled stream length
        total_out = sum(int(p.numel()) for p in parts)
        assert total_out == world * n - 1, (total_out, world * n - 1)
        del parts
        bufs = [torch.empty_like(shard_out) for _ in range(world)]      # timed leg: fixed-size RCCL all_gather per step
        for _ in range(2):
            dist.all_gather(bufs, shard_out)
        barrier()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
            dist.all_gather(bufs, shard_out)
        barrier()
        dtg = time.perf_counter() - t0
        tg = torch.tensor([dtg], dtype=torch.float64, device=cdev)
        dist.all_reduce(tg, op=dist.ReduceOp.MAX)
        extra["with_all_gather_MSamples_per_s"] = round(world * n * args.steps / float(tg[0]) / 1e6, 1)
        extra["all_gather_ms_per_step"] = round(float(tg[0]) / args.steps * 1e3, 4)
        extra["gathered_outputs"] = total_out

    if args.full and not stub:
        # sanity: the output is a demodulated 1 kHz tone of deviation 5 rad * 2 pi * 1 kHz / fs
        chk = eng.out[eng.first + 1000:eng.first + 1000 + 4096].double().cpu().numpy()
        extra["output_rms_rad"] = float(np.sqrt(np.mean(chk ** 2)))
    extra["clock_preroll"] = {"ms": args.ramp_ms, "steps": ramp_steps}
    if args.full:
        extra["first_step_ms"] = round(first_ms_max, 4)             # one-off: code object load, tap spectrum, tables
        extra["cold_ms_per_step"] = round(cold_ms_max, 4)          # steps 2..20 of the process
        extra["steady_check"] = {"steps": long_steps, "kernel_ms": round(long_ms_max, 4)}
    if per_rank is not None:
        extra["kernel_ms_per_rank"] = per_rank

    if rank == 0 or args.simulate_rank is not None:
        total = world * n * args.steps
        value = total / dt_max / 1e6
        # (one basis for the whole line: `achieved` / `frac` from the interval `value` and `ms_per_step` come from -- barrier-to-barrier wall
        #  clock over the timed steps, max over ranks; the HIP-event time of the same launches is kept beside it as kernel_ms_events)
        achieved = BYTES_PER_SAMPLE * n / (dt_max / args.steps) / 1e9
        traffic, traffic_source, power = None, None, None
        kname = eng.kernel()
        tf = os.path.join(ROOT, "profiles", "hbm_traffic.json")
        if os.path.exists(tf) and not stub:
            try:
                tj = json.load(open(tf))
                rec = tj.get("kernels", {}).get(kname) or (tj if tj.get("kernel", "").startswith(kname) else None)
                if rec:
                    traffic = rec.get("bytes_per_launch_log2n_%d" % args.log2n)
                    traffic_source = ("profiles/hbm_traffic.json (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, separate passes, "
                                      "tools/pmc_traffic.sh; not measured in this run); kernel %s at git %s"
                                      % (rec.get("kernel", kname), rec.get("git", "?")))
            except Exception:
                traffic = None
        pf = os.path.join(ROOT, "profiles", "power.json")          # rocm-smi clock / package power while the kernel loops, per kernel
        if os.path.exists(pf) and not stub:
            try:
                power = json.load(open(pf)).get("kernels", {}).get(kname)
            except Exception:
                power = None
        if args.full and world == 1 and not stub and not args.no_side:
            try:
                extra["side"] = side_configs(eng)
            except Exception as e:                        # side lines never cost the headline line
                extra["side"] = {"error": repr(e)}
        res = {
            "metric": "IQ MSamples/s through 255-tap FIR+FM demod",
            "value": round(value, 1),
            "unit": "MSamples/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(dt_max / args.steps * 1e3, 4),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "f32",
            "data": "stub" if stub else ("synthetic (ranks share one GPU)" if one_device else "synthetic"),
            "config": {"workload": "C2: 2.4 MS/s complex64 IQ (u8 grid, FM tone + noise), offsetFreq 25 kHz NCO + "
                                   "255-tap Hamming FIR + FM demod, single chunk, 2^%d samples per GPU, device resident"
                                   % args.log2n,
                       "samples_per_gpu": n, "ntaps": NTAPS, "decimation": 1,
                       "kernel_path": eng.path(), "kernel": eng.kernel(),
                       "sharding": "contiguous sample ranges, absolute-index state, no data-path collective"},
            "roofline": {"bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": traffic, "traffic_source": traffic_source,
                         "basis": "ms_per_step (wall clock between the barriers; VERDICT r5: one basis for value and frac)",
                         "kernel_ms_events": round(kern_ms_max, 4),
                         "algorithmic_bytes_per_launch": BYTES_PER_SAMPLE * n,
                         "power": power},      # (profiles/power.json: not measured in this run; says at which git revision it was)
            "extra": extra,
        }
        if args.full and not args.no_cpu_baseline and world == 1 and not stub:
            res["cpu_baseline"] = cpu_baseline(1 << args.cpu_log2n)
        print(json.dumps(res), flush=True)
    eng.close()
    if dist_on:
        dist.destroy_process_group()


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--ramp-ms", type=float, default=250.0,
                    help="untimed pre-roll of the same step before the warmup, so the measurement sees the clock the "
                         "chip holds under sustained load (the board's power controller takes ~20 ms to settle on it; "
                         "in between the kernel runs 15-35 %% slower)")
    ap.add_argument("--steady-ms", type=float, default=6000.0,
                    help="--full: device time of the steady-state check that follows the timed region (extra.steady_check)")
    ap.add_argument("--log2n", type=int, default=26, help="samples per GPU = 2^log2n")
    ap.add_argument("--full", action="store_true",
                    help="also measure and check what the headline figure does not need: first steps, steady-state check, "
                         "output sanity figure, the gather leg with more than one rank, side configurations and CPU baselines")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the decoded output of the last timed step (edges, a fixed seeded sample, the count) as DIR/<name>.npy")
    ap.add_argument("--gather", action="store_true", help="(default in a --full run with more than one rank; kept for old command lines)")
    ap.add_argument("--no-gather", action="store_true", help="--full with more than one rank: skip the RCCL all_gather leg of the decoded output")
    ap.add_argument("--force-direct", action="store_true", help="f32 direct-form kernel instead of the MFMA path")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baselines (cpu_baseline)")
    ap.add_argument("--no-side", action="store_true", help="--full: skip the C3/C4 side lines (extra.side)")
    ap.add_argument("--cpu-log2n", type=int, default=24)
    ap.add_argument("--simulate-rank", type=int, default=None,
                    help="debug: run this rank's shard (halo priming path) on one GPU without torch.distributed")
    args = ap.parse_args(argv)
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    return args


def main():
    args = parse_args()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ and args.simulate_rank is None:
        raise SystemExit(launch(args.gpus, sys.argv[1:]))
    run_rank(args)


if __name__ == "__main__":
    main()
