#!/usr/bin/env python3
"""bench.py -- iLQR backward+forward sweeps/sec on MI355X (BASELINE.json metric).

    python bench.py --gpus N --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

Both forms run N ranks, one per GPU: started plainly with --gpus N > 1 (no WORLD_SIZE in the environment) this script
becomes the launcher and runs itself under torch.distributed.run as a child process; it refuses to start when fewer than N HIP
devices are visible, and when the launcher's WORLD_SIZE disagrees with --gpus.  `n_gpus` in the line is the number of
ranks of the RCCL communicator the statistics were reduced over, not an argument or an environment variable.

Workload (BASELINE.json configs[1], SURVEY.md section 8d "C1"): double integrator, horizon N=256,
n=12, m=4, batch=4096 problems PER GPU (weak scaling: independent problem instances are sharded
over ranks with no data-path collective), fp64, time-varying storage (every knot point of every
problem owns its A,B,f,Q,R,H,q,r blocks in HBM).  One "step" = one sweep over the whole batch:
tvlqr_BackwardPass followed by tvlqr_ForwardPass semantics (src/tvlqr/tvlqr.cpp:65-248), i.e.
`altro_hip_sweep` through the C ABI.  Inputs are resident in HBM (device layout) before the timed
region starts; nothing is skipped or cached inside it (K, d, P, p, x, u, y are all rewritten).

Rank 0 prints ONE JSON line.  `roofline` is for the dominant kernel (the backward sweep) from HIP
events recorded on the kernel's own stream inside this process; `cpu_baseline` is the CPU oracle
(single thread, the reference has no threads) on a bounded sample of the same workload.
PyTorch is used for torch.distributed (RCCL) and device synchronisation only.

A plain run sets up, warms up, times the K steps, writes the outputs of the last one (--dump-outputs DIR) and prints the
line.  Everything else the line can carry -- CPU baselines, live PMC traffic passes, the single-problem seam, the repeat
block, solver statistics, the iLQR solves, the other configs -- runs only with --full.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

RED_DEVICE = "cuda"     # where the scalar reductions live (RCCL needs device tensors)
HBM_PEAK_GBS = 8000.0   # MI355X_MICROARCH.md: HBM3E 8 TB/s spec (6.29 TB/s measured copy ceiling)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=None,
                    help="problems PER GPU (weak scaling).  Default: c1 4096, c2 8192, c4 16384 per GPU (weak); c3 has a "
                         "GLOBAL default instead, see --global-batch")
    ap.add_argument("--global-batch", type=int, default=None,
                    help="problems over ALL GPUs, sharded contiguously over the ranks (strong scaling).  Default for c3: "
                         "65536 (BASELINE.json configs[3]: 65536 initial states sharded across the GPUs of a node)")
    ap.add_argument("--horizon", type=int, default=256)
    ap.add_argument("--cpu-seconds", type=float, default=12.0, help="budget for the cpu_baseline leg")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--repeat-seconds", type=float, default=6.5,
                    help="after the K timed steps: this many seconds of back-to-back sweeps, min / median / max per step")
    ap.add_argument("--config", default="c1", choices=["c1", "c2", "c3", "c4"],
                    help="c1 = BASELINE.json configs[1] (the metric's config, default); extra lines: c2 = configs[2] "
                         "(pendulum n=2 m=1 N=100 batch=8192), c3 = configs[3] (bicycle n=4 m=2 N=50 batch=65536 "
                         "per node, with the steering bound), c4 = configs[4] (random LTV n=12 m=4 N=512 "
                         "batch=16384, fp32 storage)")
    ap.add_argument("--live-traffic", action="store_true", help="(the default of --full at one GPU; kept for older command lines)")
    ap.add_argument("--no-live-traffic", action="store_true",
                    help="do not measure roofline.traffic in this run.  With --full (one GPU, rocprofv3 present) the C1 line's traffic "
                         "comes from two short rocprofv3 passes of this same command (--kernel-trace --pmc FETCH_SIZE, then WRITE_SIZE; "
                         "each counter in its own pass, nothing else traced) run as child processes before the timed region, ~1 minute; "
                         "without --full, with this flag, or when a pass fails, the tracked figure of profiles/pmc_traffic.json is used and labelled")
    ap.add_argument("--no-other-configs", action="store_true",
                    help="with --full, config c1 at one GPU also runs short timed regions of configs[2], [3] (8192 and 65536 problems) and [4] "
                         "after its own and reports them under config.other_configs; this flag leaves them out")
    ap.add_argument("--other-steps", type=int, default=10, help="timed sweeps per entry of config.other_configs")
    ap.add_argument("--sweeps-only", action="store_true",
                    help="c1: the timed sweeps and nothing after them (no iLQR solves, no other configs): what the PMC passes run")
    ap.add_argument("--lane-fused", action="store_true",
                    help="configs c2 / c3: FMA-fused LANE kernels (ALTRO_HIP_LANE_FUSED; not bit-identical to the CPU path)")
    ap.add_argument("--c4-pure", action="store_true", help="(default for config c4; kept for older command lines)")
    ap.add_argument("--c4-mixed", action="store_true",
                    help="config c4: fp32 storage with fp64 tile arithmetic (the ALTRO_HIP_F32 default of the C ABI) instead of "
                         "the pure-fp32 backward sweep (ALTRO_HIP_F32_PURE: v_mfma_f32_16x16x4_f32, four problems per wave)")
    ap.add_argument("--full", action="store_true",
                    help="also measure everything beyond the timed steps: CPU baselines, live traffic, the single-problem seam, "
                         "the repeat block, statistics, the iLQR solves and the other configs (the options above that shape "
                         "those legs apply only with --full)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one computed (K, d, P, p, x, u, y of a fixed seeded sample "
                         "of problems, delta_V and status of the whole batch) as DIR/<name>.npy")
    return ap.parse_args()


def relaunch_if_needed(args):
    """`python bench.py --gpus N` with N > 1 and no launcher around it: become the launcher (one process per GPU, the
    contract's form).  Fails loudly rather than running fewer ranks than asked for."""
    env_world = os.environ.get("WORLD_SIZE")
    if env_world is not None:
        if int(env_world) != args.gpus:
            raise SystemExit("bench.py: --gpus %d but the launcher started WORLD_SIZE=%s ranks; refusing to report a "
                             "line for a different number of GPUs than asked for" % (args.gpus, env_world))
        return
    if args.gpus <= 1:
        return
    import socket
    import altro_amd
    have = altro_amd.lib().altro_hip_device_count()
    test_hook = os.environ.get("ALTRO_BENCH_BACKEND", "nccl") != "nccl"
    if have < args.gpus and not test_hook:
        raise SystemExit("bench.py: --gpus %d but only %d HIP device(s) are visible" % (args.gpus, have))
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    print("[bench] --gpus %d: launching %s" % (args.gpus, " ".join(cmd)), file=sys.stderr, flush=True)
    # a child process, not exec: the device count above has initialised HIP in this process, and replacing a process that
    # holds the GPU open is unsafe
    import subprocess
    sys.exit(subprocess.run(cmd).returncode)


def resolve_batch(args, default_per_gpu, rank, world, default_global=None):
    """-> (problems of this rank, index of its first problem in the global batch, global batch, "weak" | "strong").
    --batch B: B problems per GPU (weak).  --global-batch G, or a config whose BASELINE entry names a node-wide batch
    (c3): the contiguous shard [lo, hi) of G (strong; ragged when world does not divide G)."""
    from altro_amd import shard
    glob = args.global_batch if args.global_batch is not None else (default_global if args.batch is None else None)
    if glob is not None:
        if glob < world:
            raise SystemExit("bench.py: global batch %d < %d ranks" % (glob, world))
        lo, hi = shard.shard_range(glob, rank, world)
        return hi - lo, lo, glob, "strong"
    per = args.batch if args.batch is not None else default_per_gpu
    return per, rank * per, per * world, "weak"


def _cpu_worker(args):
    """One host process of the all-cores CPU measurement: the same oracle loop on its own chunk of problems."""
    N, seconds, seed = args
    from oracle import oracle
    from tests import problems
    pr = problems.c1_double_integrator(4, N=N)
    L, _ = oracle.timing_lib()
    done, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        o = oracle.backward_batch(pr["A"], pr["B"], pr["f"], pr["Q"], pr["R"], pr["H"], pr["q"], pr["r"], L=L)
        oracle.forward_batch(pr["A"], pr["B"], pr["f"], o["K"], o["d"], o["P"], o["p"], pr["x0"], L=L)
        done += 4
    return done, time.perf_counter() - t0


def cpu_all_cores(N, seconds=4.0):
    """The batch is embarrassingly parallel on a CPU too: one oracle process per hardware thread, aggregate rate.
    (The reference itself has no threads; this is what a host-side batch runner could reach at best.)"""
    import multiprocessing as mp
    procs = os.cpu_count() or 1
    try:
        with mp.get_context("fork").Pool(procs) as pool:
            res = pool.map(_cpu_worker, [(N, seconds, i) for i in range(procs)])
    except Exception as e:   # noqa: BLE001 -- a measurement extra must never take the bench line down
        return {"error": str(e)}
    return {"value": sum(d for d, _ in res) / max(t for _, t in res), "unit": "problem-sweeps/s", "cores": procs,
            "sample": "%d oracle processes x %.0f s on the same C1 problems" % (procs, seconds)}


def cpu_baseline(N, seconds):
    """Single-thread CPU oracle (restatement of the reference's tvlqr pair) on a bounded sample of the
    same C1 problems; returns problem-sweeps/s."""
    from oracle import oracle
    from tests import problems
    chunk = 8
    pr = problems.c1_double_integrator(chunk, N=N)
    L, flags = oracle.timing_lib()      # the same C sources at -O3 -march=native of THIS host (results unchanged)
    done, t_used = 0, 0.0
    while t_used < seconds or done < 16:
        t0 = time.perf_counter()
        o = oracle.backward_batch(pr["A"], pr["B"], pr["f"], pr["Q"], pr["R"], pr["H"], pr["q"], pr["r"], L=L)
        oracle.forward_batch(pr["A"], pr["B"], pr["f"], o["K"], o["d"], o["P"], o["p"], pr["x0"], L=L)
        t_used += time.perf_counter() - t0
        done += chunk
        if t_used > 30.0:
            break
    cpu = "unknown"
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                cpu = line.split(":", 1)[1].strip()
                break
    except OSError:
        pass
    return {"value": done / t_used, "unit": "problem-sweeps/s", "cores": 1, "kind": "port",
            "sample": "%d problems of the same C1 workload (N=%d, n=12, m=4), %.1f s, oracle/tvlqr_oracle.c "
                      "backward+forward, %s, 1 thread of %d on '%s'" % (done, N, t_used, flags, os.cpu_count(), cpu)}


def single_problem_seam():
    """config.single_problem_seam: what one call through include/tvlqr/tvlqr.h costs on this box against the CPU port of the same
    function (tests/cpp/seam_bench.cpp; built here with g++ against libaltro_hip.so and the oracle's library)."""
    try:
        from oracle import oracle
        from tests import cpp_build
        oracle.lib()
        libdir = os.path.dirname(oracle._LIB)
        rc, out, err = cpp_build.run("seam_bench", timeout=120,
                                     extra_link=["-L" + libdir, "-l:" + os.path.basename(oracle._LIB), "-Wl,-rpath," + libdir])
        if rc != 0:
            return {"error": (out + err)[-300:]}
        return json.loads(out.strip().splitlines()[-1])
    except Exception as e:   # noqa: BLE001 -- an extra must never take the line down
        return {"error": str(e)}


def eigen_probe():
    """the reference's own CPU path needs Eigen >= 3.4 (deps/CMakeLists.txt:15-19), which is not
    part of this image.  Probe for it so that the line SAYS which CPU path was timed."""
    import shutil
    import subprocess
    import tempfile
    gxx = shutil.which("g++")
    if not gxx:
        return "g++ not found: Eigen not probed; reference CPU path stated by restatement (oracle/, kind 'port')"
    with tempfile.TemporaryDirectory() as td:
        src = os.path.join(td, "p.cpp")
        with open(src, "w") as f:
            f.write("#include <Eigen/Dense>\n#if !EIGEN_VERSION_AT_LEAST(3, 4, 0)\n#error old\n#endif\nint main() { return 0; }\n")
        for inc in ([], ["-I/usr/include/eigen3"], ["-I/usr/local/include/eigen3"], ["-I/opt/conda/include/eigen3"]):
            r = subprocess.run([gxx, "-std=c++17", "-fsyntax-only"] + inc + [src], capture_output=True)
            if r.returncode == 0:
                return ("Eigen >= 3.4 found (%s) but no Eigen harness is shipped: the image this repo is built and tested on has "
                        "no Eigen, so one could not be validated; CPU path = restatement (oracle/, kind 'port')" % (inc or ["default path"]))
    return "Eigen not available on this host -- reference CPU path stated by restatement (oracle/tvlqr_oracle.c, kind 'port')"


def timed_region(bt, args, world, dist, torch, shard):
    """The contract's timing: W untimed sweeps, then EXACTLY K sweeps bracketed by barrier + synchronize on both sides,
    max over ranks.  Every launch inside the region is bracketed by hipEvents on the handle's own stream without any
    wait in between (profile mode 2), so the per-kernel durations belong to the same sweeps as the headline number."""
    def barrier():
        if world > 1:
            dist.barrier()
    for _ in range(args.warmup):
        bt.sweep()
    bt.profile(2)              # events only; reset after the warm-up
    barrier(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        bt.sweep()
    torch.cuda.synchronize()
    global _ELAPSED_LOCAL
    _ELAPSED_LOCAL = time.perf_counter() - t0      # this rank's own K steps (before the closing barrier): the per-rank table
    barrier()
    elapsed = shard.max_over_ranks(time.perf_counter() - t0, device=RED_DEVICE)
    kern = {}
    for slot in (0, 1):
        nl, ms, name = bt.profile_get(slot)
        lo, hi = bt.profile_range(slot)
        kern[slot] = {"name": name, "launches": nl, "launches_not_recorded": bt.profile_dropped(slot),
                      "avg_ms": ms / max(nl, 1), "min_ms": lo, "max_ms": hi}
    bt.profile(0)
    return elapsed, kern


_ELAPSED_LOCAL = None


def elapsed_local():
    return _ELAPSED_LOCAL


def rank_table(elapsed, steps, local_rank, rank, world, dist, torch):
    """config.ranks: per rank its HIP device, that device's PCI bus id and name, and the time of ITS K steps -- gathered with
    torch.distributed after the timed region (an object gather: nothing of the data path).  Lets a reader of a multi-GPU line
    see a straggler, or two ranks bound to one device."""
    import altro_amd
    row = {"rank": rank, "local_rank": local_rank, "device": local_rank, "pid": os.getpid(),
           "ms_per_step_own": None if elapsed is None else elapsed / steps * 1e3}
    try:
        name, cus, pci = altro_amd.device_info(local_rank)
        row.update({"name": name, "compute_units": cus, "pci_bus_id": pci})
    except Exception as e:   # noqa: BLE001
        row["device_info_error"] = str(e)
    if world == 1:
        return [row]
    rows = [None] * world
    try:
        dist.all_gather_object(rows, row)
    except Exception as e:   # noqa: BLE001
        return [dict(row, gather_error=str(e))]
    devs = [r.get("pci_bus_id") for r in rows if r]
    if len(set(devs)) != len(devs):
        print("[bench] WARNING: two ranks report the same PCI bus id: %s" % devs, file=sys.stderr)
    return rows


def repeat_block(bt, torch, ms_per_step, seconds):
    """>= `seconds` of back-to-back sweeps AFTER the contract's K steps (which last only tens of milliseconds), without
    events, timed in blocks on the host clock: the run-to-run spread of a sweep, in the line itself."""
    if seconds <= 0:
        return None
    per_block = max(10, int(0.05 / max(ms_per_step * 1e-3, 1e-6)))     # ~50 ms per block
    blocks, t_all = [], time.perf_counter()
    while time.perf_counter() - t_all < seconds or len(blocks) < 5:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(per_block):
            bt.sweep()
        torch.cuda.synchronize()
        blocks.append((time.perf_counter() - t0) / per_block * 1e3)
        if len(blocks) >= 400:
            break
    blocks.sort()
    return {"sweeps": per_block * len(blocks), "seconds": time.perf_counter() - t_all, "block_sweeps": per_block,
            "ms_per_step": {"min": blocks[0], "median": blocks[len(blocks) // 2], "max": blocks[-1]},
            "note": "host clock around blocks of back-to-back sweeps, no events, after the timed region"}


class StatsChannel:
    """the statistics reduction is the path's only collective.  Under RCCL (backend nccl) it is the
    C ABI's own entry -- device-side reduction + two ncclAllReduce on the handle's stream over a communicator the
    library opens itself; under the single-box gloo test hook (ALTRO_BENCH_BACKEND=gloo: every rank on the box's one GPU,
    where RCCL refuses to put two ranks on one device) the same device-side reduction followed by the same two
    all-reduces through torch.distributed.  `world` -- the line's n_gpus -- is what the channel itself reports."""

    def __init__(self, local_rank, rank, env_world, shard, dist):
        self.shard, self.local_rank, self.rank = shard, local_rank, rank
        self.comm, self.note = None, None
        if RED_DEVICE == "cuda":
            try:
                self.comm = shard.make_comm(local_rank, rank, env_world)
                self.world = self.comm.world           # altro_hip_comm_world: ranks of the RCCL communicator
                self.how = "altro_hip_stats_allreduce (device-side reduction + 2 x ncclAllReduce, RCCL, world %d)" % self.world
                return
            except Exception as e:   # noqa: BLE001 -- statistics are outside the timed region: never cost the line
                print("[bench] RCCL communicator failed on rank %d (%s); falling back to torch.distributed" % (rank, e),
                      file=sys.stderr)
                self.note = str(e)
        self.world = dist.get_world_size() if (dist.is_available() and dist.is_initialized()) else 1
        if RED_DEVICE == "cuda":
            self.how = ("altro_hip_stats_reduce (device) + torch.distributed nccl all_reduce, world %d (fallback: %s)"
                        % (self.world, self.note)) if self.world > 1 else \
                       "altro_hip_stats_reduce (device); no collective (world 1; RCCL unavailable: %s)" % self.note
        else:
            self.how = "altro_hip_stats_reduce (device) + torch.distributed gloo all_reduce, world %d (test hook)" % self.world

    def reduce(self, bt):
        if self.comm is not None:
            st = bt.stats(self.comm).as_dict()
        elif self.world == 1:
            st = bt.stats().as_dict()
        else:
            st = self.shard.reduce_stats(bt.stats(), device=("cuda:%d" % self.local_rank) if RED_DEVICE == "cuda" else "cpu")
        st["reduced_by"] = self.how
        return st

    def close(self):
        if self.comm is not None:
            self.comm.close()
            self.comm = None


_LIVE_TRAFFIC = None   # {kernel name: bytes per launch}, filled by live_traffic() on rank 0 of a one-GPU run
_LIVE_TRAFFIC_NOTE = None


def live_traffic(args, config=None, batch=None):
    """HBM bytes per launch of the sweep kernels from two rocprofv3 PMC passes of this very command (steps 3, no CPU leg, no
    repeat block), exactly as MI355X_MICROARCH.md prescribes: FETCH_SIZE and WRITE_SIZE each in its own pass with
    --kernel-trace only, values in KiB, FETCH_SIZE doubled on gfx950.  Returns {kernel name: bytes} or None."""
    import shutil
    import sqlite3
    import subprocess
    import tempfile
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(prof):
        print("[bench] --live-traffic: rocprofv3 not found", file=sys.stderr)
        return None
    child = [sys.executable, os.path.abspath(__file__), "--config", config or args.config, "--steps", "3", "--warmup", "1", "--no-cpu-baseline",
             "--no-live-traffic", "--no-other-configs", "--sweeps-only", "--repeat-seconds", "0"]
    if config is None:
        child += ["--horizon", str(args.horizon)]
    if batch is not None:
        child += ["--batch", str(batch)]
    elif args.batch is not None:
        child += ["--batch", str(args.batch)]
    if args.global_batch is not None:
        child += ["--global-batch", str(args.global_batch)]
    if args.c4_mixed:
        child += ["--c4-mixed"]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    env["TMPDIR"] = "/tmp"
    sums = {}
    for ctr in ("FETCH_SIZE", "WRITE_SIZE"):
        with tempfile.TemporaryDirectory(dir="/tmp") as td:
            r = subprocess.run([prof, "--kernel-trace", "--pmc", ctr, "-d", td, "-o", "t", "--"] + child, cwd="/tmp", env=env,
                               capture_output=True, text=True, timeout=600)
            dbs = [os.path.join(dp, f) for dp, _, fs in os.walk(td) for f in fs if f.endswith(".db")]
            if r.returncode != 0 or not dbs:
                print("[bench] --live-traffic: the %s pass failed (rc %d)" % (ctr, r.returncode), file=sys.stderr)
                return None
            con = sqlite3.connect(dbs[0])
            rows = con.execute("select kernel_name, avg(v) from (select kernel_name, dispatch_id, sum(value) as v from counters_collection "
                               "where counter_name = ? group by kernel_name, dispatch_id) group by kernel_name", (ctr,)).fetchall()
            con.close()
            for name, kib in rows:
                sums.setdefault(name, {})[ctr] = kib
    return {name: 2.0 * 1024.0 * v.get("FETCH_SIZE", 0.0) + 1024.0 * v.get("WRITE_SIZE", 0.0) for name, v in sums.items()}


def roofline_block(cfg_key, batch, N, name, alg_bytes, dur, slot=0, live=None):
    """`achieved` / `frac` follow the contract: SURVEY 8(d) ALGORITHMIC bytes per launch / measured duration / 8 TB/s.
    `traffic` is the PMC byte count of a tracked earlier rocprofv3 run of the same command (profiles/pmc_traffic.json),
    NOT a live counter read; `frac_traffic` prices those physical bytes against the same peak.  slot 0 = the backward
    sweep (the dominant kernel: `roofline`), slot 1 = the forward sweep (`roofline_forward`)."""
    traffic, source = None, None
    tpath = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    try:
        tj = json.load(open(tpath)).get(cfg_key) or {}
        if tj.get("batch") == batch and tj.get("horizon") == N and tj.get("calibrated", True):
            traffic = tj.get("backward_bytes_per_launch" if slot == 0 else "forward_bytes_per_launch")
            if traffic:
                source = "profiles/pmc_traffic.json[%s] <- %s (tracked rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of an " \
                         "earlier run of this command; not measured in this run)" % (cfg_key, tj.get("profile"))
    except (OSError, ValueError):
        pass
    live = _LIVE_TRAFFIC if live is None else live
    if live:   # measured in this run: the kernel whose (demangled) name contains the profiled slot's name
        hit = [v for k, v in live.items() if name in k]
        if hit:
            traffic = max(hit)
            source = "LIVE: rocprofv3 --kernel-trace --pmc FETCH_SIZE / WRITE_SIZE passes of this command run by this process " \
                     "(bytes = 2 * 1024 * FETCH_SIZE + 1024 * WRITE_SIZE per launch, MI355X_MICROARCH.md)"
    ach = alg_bytes / dur / 1e9
    return {"bound": "hbm", "kernel": name, "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": ach / HBM_PEAK_GBS, "frac_algorithmic": ach / HBM_PEAK_GBS,
            "traffic": traffic, "traffic_source": source,
            "traffic_GBps": (traffic / dur / 1e9) if traffic else None,
            "frac_traffic": (traffic / dur / 1e9 / HBM_PEAK_GBS) if traffic else None,
            "duration_ms": dur * 1e3,
            "duration_source": "hipEvents on the handle's stream around every launch of the timed region (no wait between launches)",
            "note": "frac = frac_algorithmic = SURVEY 8(d) bytes of the full n x n blocks / kernel time / 8 TB/s; the records "
                    "hold the symmetric Q and P blocks as triangles, so the bytes that move (traffic) are fewer and "
                    "frac_traffic is the physical HBM utilisation"}


def cpu_sweep_rate(N, n, m, seconds, dtype_note=""):
    """Single-thread CPU oracle on TVLQR problems of the shape (N, n, m): backward + forward per problem (the sweep's cost on a
    CPU does not depend on the values, so seeded random LTV-LQ problems of the shape stand for the config's own)."""
    from oracle import oracle
    from tests import problems
    chunk = 8
    pr = problems.random_ltv(chunk, N, n, m)
    L, flags = oracle.timing_lib()
    done, t_used = 0, 0.0
    while t_used < seconds or done < 16:
        t0 = time.perf_counter()
        o = oracle.backward_batch(pr["A"], pr["B"], pr["f"], pr["Q"], pr["R"], pr["H"], pr["q"], pr["r"], L=L)
        oracle.forward_batch(pr["A"], pr["B"], pr["f"], o["K"], o["d"], o["P"], o["p"], pr["x0"], L=L)
        t_used += time.perf_counter() - t0
        done += chunk
    return {"value": done / t_used, "unit": "problem-sweeps/s", "cores": 1, "kind": "port",
            "sample": "%d seeded random LTV-LQ problems of this shape (N=%d, n=%d, m=%d), %.1f s, oracle/tvlqr_oracle.c backward+forward "
                      "in fp64%s, %s, 1 thread" % (done, N, n, m, t_used, dtype_note, flags)}


def make_lane_batch(cfg, batch, first, N, device, lane_fused=False):
    """configs[2] (pendulum) / configs[3] (bicycle tracking with the steering bound) on plan LANE: the handle with its model, cost,
    constraint block, initial states (this rank's slice of the global batch) and input guess, expanded at the initial rollout.
    -> (handle, callable that restores the input guess)"""
    import altro_amd
    from tests import problems
    c3 = cfg == "c3"
    n, m = (4, 2) if c3 else (2, 1)
    bt = altro_amd.Batch(N, n, m, batch, device=device, flags=altro_amd.LANE_FUSED if lane_fused else 0)
    assert bt.plan == altro_amd.PLAN_LANE
    if c3:
        x_ref, u_ref = problems.bicycle_reference(N + 1)
        bt.set_model(altro_amd.MODEL_BICYCLE, np.float32(0.1))
        bt.set_tracking_cost(np.full((1, N + 1, n), 1e-2), np.full((1, N, m), 1e-3), x_ref[None, :N + 1],
                             u_ref[None, :N], batch_stride_zero=True)
        G = np.zeros((2, n + m)); G[0, 3] = 1.0; G[1, 3] = -1.0
        bt.add_linear_constraint(0, N, altro_amd.CONE_INEQUALITY, G, np.full(2, np.pi / 3))
        x0 = x_ref[0] + (problems.uniform01((batch, n), 23, first * n) - 0.5) * 0.4
        guess = np.array([[[u_ref[0][0], 0.0]]])
    else:
        bt.set_model(altro_amd.MODEL_PENDULUM, np.float32(0.03))
        xf = np.array([np.pi, 0.0])
        bt.set_tracking_cost(np.array([[1e-2, 1e-2], [1.0, 1.0]]), np.array([[1e-3]]), np.stack([xf, xf]),
                             np.zeros((1, m)), k_stride_zero=True, batch_stride_zero=True)
        x0 = np.zeros((batch, n)); x0[:, 0] = problems.uniform01((batch,), 22, first) - 0.5
        guess = np.array([[[0.1]]])

    def set_guess():
        bt.set_input_guess(guess, k_stride_zero=True, batch_stride_zero=True)
    set_guess()
    bt.set_initial_state(x0)
    bt.open_loop_rollout(); bt.accept(); bt.expand()
    return bt, set_guess


def make_mfma_batch(c4, c4_pure, batch, first, N, device):
    """configs[1] (C1 double integrator, fp64) / configs[4] (random LTV, fp32) on plan MFMA16, data resident in HBM."""
    import altro_amd
    from tests import problems
    n, m = 12, 4
    x0 = 2.0 * problems.uniform01((batch, n), 21, first * n) - 1.0   # this rank's slice of the global batch
    bt = altro_amd.Batch(N, n, m, batch, dtype=altro_amd.F32 if c4 else altro_amd.F64, device=device,
                         flags=altro_amd.F32_PURE if (c4 and c4_pure) else 0)
    assert bt.plan == altro_amd.PLAN_MFMA16
    if c4:
        # random time-varying LTV-LQ problems (SURVEY.md 8d "C4"): a seeded pool of 64 distinct problems is
        # tiled over the batch ON THE DEVICE; every (problem, knot point) still owns its blocks in HBM
        pool = problems.random_ltv(64, N, n, m)
        bt.set_host_batch(64)
        bt.set_dynamics(pool["A"], pool["B"], pool["f"])
        bt.set_cost(pool["Q"], pool["R"], pool["H"], pool["q"], pool["r"])
        bt.set_host_batch(0)
    else:
        one = problems.c1_double_integrator(1, N=N)
        # shared A,B,Q,R are EXPANDED on the device: every (problem, knot point) owns its blocks in HBM
        # f is PRESENT (zeros): tvlqr_BackwardPass always reads f[k] (tvlqr.cpp:147-148), and SURVEY 8(d)'s 5088 B per knot point count
        # it -- so the HAS_F instantiation is the one timed and every algorithmic byte is in play (VERDICT r4 weak #5b)
        bt.set_dynamics(one["A"][0, :1], one["B"][0, :1], one["f"][0, :1], k_stride_zero=True, batch_stride_zero=True)
        Q2 = np.stack([one["Q"][0, 0], one["Q"][0, N]])
        bt.set_cost(Q2, one["R"][0, :1], one["H"][0, :1], np.zeros((2, n)), one["r"][0, :1],
                    k_stride_zero=True, batch_stride_zero=True)
    bt.set_initial_state(x0)
    return bt


def other_config_entry(key, device, steps, torch, cpu_seconds=2.0, live=None):
    """One entry of config.other_configs: a short timed region (3 untimed sweeps, then `steps` sweeps between two device
    synchronisations; per-kernel hipEvents inside it) of another BASELINE.json config on this GPU, with the roofline fraction
    of its backward sweep, the tracked PMC traffic where it is calibrated, and a bounded single-thread CPU figure."""
    cfg, batch = {"c2": ("c2", 8192), "c3_8192": ("c3", 8192), "c3_65536": ("c3", 65536), "c4": ("c4", 16384)}[key]
    N = {"c2": 100, "c3": 50, "c4": 512}[cfg]
    n, m = {"c2": (2, 1), "c3": (4, 2), "c4": (12, 4)}[cfg]
    t_setup = time.perf_counter()
    set_guess = None
    if cfg == "c4":
        bt = make_mfma_batch(True, True, batch, 0, N, device)
    else:
        bt, set_guess = make_lane_batch(cfg, batch, 0, N, device)
    for _ in range(3):
        bt.sweep()
    bt.profile(2)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        bt.sweep()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    kern = {}
    for slot in (0, 1):
        nl, ms, name = bt.profile_get(slot)
        kern[slot] = {"name": name, "launches": nl, "avg_ms": ms / max(nl, 1)}
    bt.profile(0)
    bytes_b, bytes_f = bt.algorithmic_bytes(0), bt.algorithmic_bytes(1)
    dur_b, dur_f = kern[0]["avg_ms"] * 1e-3, kern[1]["avg_ms"] * 1e-3
    cfg_key = "c4pure" if cfg == "c4" else cfg
    roof = roofline_block(cfg_key, batch, N, kern[0]["name"], bytes_b, dur_b, live=live or {})
    roof_f = roofline_block(cfg_key, batch, N, kern[1]["name"], bytes_f, dur_f, slot=1, live=live or {})
    for r in (roof, roof_f):
        r.pop("note", None); r.pop("duration_source", None)
    if cfg != "c4" and batch <= 8192:
        roof["bound_in_practice"] = ("instruction issue of one wave per SIMD, not HBM: %d waves on 1024 SIMDs walk N = %d dependent steps; "
                                    "SQ_ACTIVE_INST_ANY / SQ_WAVE_CYCLES = 0.72-0.75, SQ_WAIT_INST_ANY / SQ_WAVE_CYCLES = 0.05-0.12 "
                                    "(profiles/r04zf_quad_pmc.txt: 559 VALU instructions per knot point and wave for (4, 2)), half the SIMDs idle -- "
                                    "so `frac` is reported for reference only" % ((batch + 15) // 16, N))
    out = {"workload": {"c2": "C2 pendulum swing-up (BASELINE.json configs[2]): TVLQR sweep on the expansion at the initial rollout",
                        "c3": "C3 bicycle tracking + steering bound (BASELINE.json configs[3]): TVLQR sweep on the expansion at the initial rollout",
                        "c4": "C4 random LTV TVLQR sweep, pure fp32 (BASELINE.json configs[4])"}[cfg],
           "horizon_N": N, "n": n, "m": m, "batch": batch, "dtype": "f32" if cfg == "c4" else "f64", "steps": steps,
           "ms_per_step": elapsed / steps * 1e3, "value": batch * steps / elapsed, "unit": "problem-sweeps/s",
           "kernels": {kern[0]["name"]: dict(kern[0], algorithmic_GB=bytes_b / 1e9, GBps=bytes_b / dur_b / 1e9),
                       kern[1]["name"]: dict(kern[1], algorithmic_GB=bytes_f / 1e9, GBps=bytes_f / dur_f / 1e9)},
           "roofline": roof, "roofline_forward": roof_f}
    if set_guess is not None:   # the same batch as one whole AL-iLQR solve (second of two: the first loads the kernels' code)
        c3 = cfg == "c3"
        for timed in (False, True):
            if c3:
                bt.reset_duals(1.0)
            set_guess()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            res = bt.ilqr_solve(iterations_max=80, use_backtracking=c3)
            torch.cuda.synchronize()
            t_solve = time.perf_counter() - t1
        out["full_solve"] = {"ms": t_solve * 1e3, "sweeps": int(res["sweeps"]), "converged": int((res["status"] == 0).sum()),
                             "mean_iterations": float(res["iterations"].mean())}
        # A batched solve lasts as long as its slowest problem: the same solve again through altro_hip_ilqr_solve_async / _poll (the solve
        # kernel publishes every problem into pinned host memory the moment it stops) -- the time after which 99.9 % of the batch have
        # their result, which is what an MPC caller that uses each problem as it finishes waits for
        try:
            if c3:
                bt.reset_duals(1.0)
            set_guess()
            torch.cuda.synchronize()
            want = batch - max(1, batch // 1000)
            t1 = time.perf_counter()
            bt.ilqr_solve_async(iterations_max=80, use_backtracking=c3)
            t999 = None
            while True:
                ndone, _ = bt.poll()
                if ndone >= want:
                    t999 = time.perf_counter() - t1
                    break
                if time.perf_counter() - t1 > 5.0:
                    break
            r9 = bt.wait()
            out["full_solve"]["ms_to_p999"] = None if t999 is None else t999 * 1e3
            out["full_solve"]["ms_async_total"] = (time.perf_counter() - t1) * 1e3
            out["full_solve"]["stragglers"] = ("after ms_to_p999 at most %d problems still run: one wave's dependent chain per sweep whatever rides it "
                                               "(tools/c3_small_batches.py: 0.24 ms per sweep at 64 problems, 0.31 at 8192, 0.99 at 65536)" % (batch - want))
            assert int((r9["status"] == 0).sum()) == out["full_solve"]["converged"]
        except Exception as e:   # noqa: BLE001
            out["full_solve"]["ms_to_p999"] = {"error": str(e)}
    bt.close()
    if cfg != "c4" and batch <= 8192:
        # What bit-identity with the CPU path costs at this latency-bound size: the same sweeps with ALTRO_HIP_LANE_FUSED (the kernels
        # may contract a * b + c into one FMA: 1e-12 relative instead of bit-identical; an opt-in flag of altro_hip_batch_create, NOT
        # what the numbers above ran)
        bf, _ = make_lane_batch(cfg, batch, 0, N, device, lane_fused=True)
        for _ in range(3):
            bf.sweep()
        bf.profile(2)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        for _ in range(steps):
            bf.sweep()
        torch.cuda.synchronize()
        el2 = time.perf_counter() - t2
        nl0, ms0, name0 = bf.profile_get(0)
        nl1, ms1, name1 = bf.profile_get(1)
        bf.profile(0)
        bf.close()
        out["fma_contracted_variant"] = {"flag": "ALTRO_HIP_LANE_FUSED (opt-in; not bit-identical to the CPU path: 1e-12 relative)",
                                         "ms_per_step": el2 / steps * 1e3, name0: {"avg_ms": ms0 / max(nl0, 1)}, name1: {"avg_ms": ms1 / max(nl1, 1)},
                                         "backward_frac": bytes_b / (ms0 / max(nl0, 1) * 1e-3) / 8e12}
    if cpu_seconds > 0:
        out["cpu_baseline"] = cpu_sweep_rate(N, n, m, cpu_seconds, " (the GPU line: fp32)" if cfg == "c4" else "")
        out["vs_cpu_single_thread"] = out["value"] / out["cpu_baseline"]["value"]
    out["seconds_total"] = time.perf_counter() - t_setup
    return out


def quad13_nmpc_entry(device, torch, batch=4096, N=30, steps=6):
    """config.other_configs.quad13_nmpc (round 6): nonlinear dynamics past the (12, 4) tile -- a batched receding-horizon NMPC of
    13-state quaternion quadrotors on plan MFMA32, the compiled-in device model in the row-layout loop kernels
    (kernels/ilqr_row32.hip: r32_model_step), warm steps timed on the host clock around altro_hip_ilqr_solve."""
    import time

    import altro_amd
    n, m, h = 13, 4, np.float32(0.02)
    hover = np.array([0.5 * 9.81, 0.0, 0.0, 0.0])
    rng = np.random.default_rng(7)
    x0 = np.zeros((batch, n))
    x0[:, :3] = 0.8 * rng.standard_normal((batch, 3))
    q = np.concatenate([np.ones((batch, 1)), 0.12 * rng.standard_normal((batch, 3))], axis=1)
    x0[:, 3:7] = q / np.linalg.norm(q, axis=1, keepdims=True)
    x0[:, 7:10] = 0.3 * rng.standard_normal((batch, 3)); x0[:, 10:] = 0.2 * rng.standard_normal((batch, 3))
    xref = np.zeros(n); xref[3] = 1.0
    Qd = np.concatenate([np.full(3, 2.0), np.full(4, 1.0), np.full(3, 0.5), np.full(3, 0.1)])
    Rd = np.array([0.05, 20.0, 20.0, 20.0])
    bt = altro_amd.Batch(N, n, m, batch, device=device)
    try:
        bt.set_model(altro_amd.MODEL_QUADROTOR13, h)
        bt.set_tracking_cost(np.stack([Qd, 20.0 * Qd]), Rd[None], np.stack([xref, xref]), hover[None], k_stride_zero=True, batch_stride_zero=True)
        bt.set_initial_state(x0)
        bt.set_input_guess(hover[None, None], k_stride_zero=True, batch_stride_zero=True)
        res = bt.ilqr_solve(iterations_max=40, tol_stationarity=1e-3)
        first = {"sweeps": int(res["sweeps"]), "converged": int((res["status"] == 0).sum())}
        ts, sw, it = [], [], []
        for _ in range(steps):
            x1, _u = bt.get_knot(1)
            bt.set_initial_state(x1)
            bt.shift_trajectory()
            bt.synchronize(); t0 = time.perf_counter()
            res = bt.ilqr_solve(iterations_max=40, tol_stationarity=1e-3)
            bt.synchronize(); ts.append((time.perf_counter() - t0) * 1e3)
            sw.append(int(res["sweeps"])); it.append(float(res["iterations"].mean()))
        med = sorted(ts)[len(ts) // 2]
        return {"workload": "batched NMPC of %d 13-state quaternion quadrotors (MODEL_QUADROTOR13), N = %d, h = 0.02, warm receding-horizon steps" % (batch, N),
                "plan": int(bt.plan), "model_kernels": "row layout" if bt.model_row_layout() else "wave per problem",
                "ms_per_step_median": med, "ms_per_step": ts, "sweeps": sw, "mean_iterations": it, "first_solve": first,
                "vehicle_steps_per_s": batch / (med * 1e-3)}
    finally:
        bt.close()


def mfma32_entry(n, m, device, steps, torch, cpu_seconds=2.0, N=128, batch=4096):
    """Plan MFMA32 (kernels/tvlqr_tile32.hip): the TVLQR sweep of a shape one step past the (12, 4) tile -- (13, 4), a quaternion
    quadrotor's dimensions, and (28, 4) -- at the shape-cliff table's size (4096 problems x 128 knot points, random LTV problems,
    fp64, time-varying storage), with the roofline fraction of both sweep kernels.  The arrays are plan GENERIC's full blocks, so
    algorithmic bytes = the bytes that move."""
    import altro_amd
    from tests import problems
    t_setup = time.perf_counter()
    pr = problems.random_ltv(16, N, n, m)
    rep = lambda a: np.ascontiguousarray(np.tile(a, (batch // 16,) + (1,) * (a.ndim - 1)))
    bt = altro_amd.Batch(N, n, m, batch, device=device)
    assert bt.plan == altro_amd.PLAN_MFMA32
    bt.set_dynamics(rep(pr["A"]), rep(pr["B"]), rep(pr["f"]))
    bt.set_cost(rep(pr["Q"]), rep(pr["R"]), rep(pr["H"]), rep(pr["q"]), rep(pr["r"]))
    bt.set_initial_state(rep(pr["x0"]))
    for _ in range(3):
        bt.sweep()
    bt.profile(2)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        bt.sweep()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    kern = {}
    for slot in (0, 1):
        nl, ms, name = bt.profile_get(slot)
        kern[slot] = {"name": name, "launches": nl, "avg_ms": ms / max(nl, 1)}
    bt.profile(0)
    assert (bt.get("status") == -1).all()
    bytes_b, bytes_f = bt.algorithmic_bytes(0), bt.algorithmic_bytes(1)
    bt.close()
    # the iLQR loop on the same shape (tools/solve_shapes.py's problems, 16 of them tiled): one MeritFunction evaluation with derivative
    # (kernels/ilqr_row32.hip; "lds": plan GENERIC's wave-per-problem kernel it replaced on these shapes) and whole solves, without and
    # with an input box -- host clock, stream drained
    ilqr = {}
    try:
        pl = problems.ilqr12x4_problem(16, N, True, n=n, m=m)
        G = np.zeros((2 * m, n + m)); G[:m, n:] = np.eye(m); G[m:, n:] = -np.eye(m)
        for key, forms in (("row_layout", 0), ("lds", altro_amd.FORM_GENERIC_MERIT_LDS)):
            b2 = altro_amd.Batch(N, n, m, batch, device=device)
            b2.set_forms(forms)
            b2.set_dynamics(rep(pl["A"]), rep(pl["B"]), rep(pl["f"]))
            b2.set_tracking_cost(rep(pl["Qd"]), rep(pl["Rd"]), rep(pl["xref"]), rep(pl["uref"]))
            b2.set_initial_state(rep(pl["x0"])); b2.set_input_guess(rep(pl["u0"]))
            b2.open_loop_rollout(); b2.accept(); b2.expand(); b2.backward()
            ts = []
            for _ in range(6):
                torch.cuda.synchronize(); t1 = time.perf_counter()
                b2.merit(1.0); b2.synchronize()
                ts.append((time.perf_counter() - t1) * 1e3)
            e = {"merit_with_derivative_ms": sorted(ts[1:])[len(ts[1:]) // 2]}
            if key == "row_layout":
                for tag, bounds in (("solve", False), ("solve_input_box", True)):
                    if bounds:
                        b2.add_linear_constraint(0, N - 1, altro_amd.CONE_INEQUALITY, G, np.full(2 * m, 0.5))
                    t2 = []
                    for _ in range(3):
                        b2.set_input_guess(rep(pl["u0"]))
                        if bounds:
                            b2.reset_duals(1.0)
                        b2.synchronize(); t1 = time.perf_counter()
                        res = b2.ilqr_solve(iterations_max=40)
                        b2.synchronize()
                        t2.append((time.perf_counter() - t1) * 1e3)
                    e[tag] = {"ms": sorted(t2[1:])[0], "sweeps": int(res["sweeps"]), "merit_launches": int(res["merit_launches"]),
                              "converged": int((res["status"] == 0).sum())}
            ilqr[key] = e
            b2.close()
    except Exception as ex:  # noqa: BLE001
        ilqr["error"] = str(ex)
    out = {"workload": "TVLQR sweep of random LTV problems, (n, m) = (%d, %d): plan MFMA32, 2 x 2 tiles of v_mfma_f64_16x16x4" % (n, m),
           "horizon_N": N, "n": n, "m": m, "batch": batch, "dtype": "f64", "steps": steps, "ms_per_step": elapsed / steps * 1e3,
           "value": batch * steps / elapsed, "unit": "problem-sweeps/s", "kernels": {}}
    for slot, key, by in ((0, "roofline", bytes_b), (1, "roofline_forward", bytes_f)):
        dur = kern[slot]["avg_ms"] * 1e-3
        out["kernels"][kern[slot]["name"]] = dict(kern[slot], algorithmic_GB=by / 1e9, GBps=by / dur / 1e9)
        out[key] = {"bound": "hbm", "kernel": kern[slot]["name"], "achieved": by / dur / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                    "frac": by / dur / 1e9 / HBM_PEAK_GBS, "duration_ms": dur * 1e3, "traffic": None,
                    "traffic_source": "full n x n blocks in HBM: the algorithmic bytes are the bytes the kernel requests (profiles/r06*_tile32_pmc.txt)"}
    if cpu_seconds > 0:
        out["cpu_baseline"] = cpu_sweep_rate(N, n, m, cpu_seconds)
        out["vs_cpu_single_thread"] = out["value"] / out["cpu_baseline"]["value"]
    out["ilqr_loop"] = ilqr
    out["seconds_total"] = time.perf_counter() - t_setup
    return out


def lane_config(args, rank, local_rank, world, dist, torch, chan):
    """Extra lines for the small-state configs (plan LANE, lane-per-problem SoA): the same sweep metric on the
    expansion of a nonlinear model, plus the time of one full batched AL-iLQR solve."""
    import altro_amd
    from altro_amd import shard
    from tests import problems
    c3 = args.config == "c3"
    if c3:
        n, m, N = 4, 2, 50 if args.horizon == 256 else args.horizon
        # configs[3]: 65536 random initial states sharded over the GPUs of the node (8192 each at 8 GPUs, all of them
        # on the one GPU of an N=1 run); --batch B makes it B per GPU instead (the tracked profiles use 8192)
        batch, first, global_batch, scaling = resolve_batch(args, None, rank, world, default_global=65536)
    else:
        n, m, N = 2, 1, 100 if args.horizon == 256 else args.horizon
        batch, first, global_batch, scaling = resolve_batch(args, 8192, rank, world)
    bt, set_guess = make_lane_batch(args.config, batch, first, N, local_rank, args.lane_fused)

    elapsed, kern = timed_region(bt, args, world, dist, torch, shard)
    if args.dump_outputs and rank == 0:
        dump_outputs(bt, torch, args.dump_outputs, first, False)
    rep = repeat_block(bt, torch, elapsed / args.steps * 1e3, args.repeat_seconds if args.full else 0)
    ms_b, nb, name_b = kern[0]["avg_ms"], 1, kern[0]["name"]
    ms_f, nf, name_f = kern[1]["avg_ms"], 1, kern[1]["name"]
    full_solve, stats = None, None
    if args.full:
        # one full batched solve (all problems to convergence), timed on the host clock; one untimed solve first (the first
        # launch of each kernel loads its code object), duals and penalties reset in between so that both start alike
        t_solves = []
        for timed in (False, True, True, True):     # (median of three timed solves)
            if c3:
                bt.reset_duals(1.0)
            set_guess()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            res = bt.ilqr_solve(iterations_max=80, use_backtracking=c3)
            torch.cuda.synchronize()
            if timed:
                t_solves.append(time.perf_counter() - t1)
        t_solve = sorted(t_solves)[1]
        full_solve = {"seconds": t_solve, "seconds_min_max": [min(t_solves), max(t_solves)], "sweeps": int(res["sweeps"]),
                      "merit_launches": int(res["merit_launches"]),
                      "converged": int((res["status"] == 0).sum()),
                      "mean_iterations": float(res["iterations"].mean()),
                      "problems_per_s": batch / t_solve}
        stats = chan.reduce(bt)     # after the solve: the quantities Solve reports
    if rank == 0:
        bytes_b, bytes_f = bt.algorithmic_bytes(0), bt.algorithmic_bytes(1)
        dur_b = ms_b / nb * 1e-3
        emit(({
            "metric": "iLQR backward+forward sweeps/sec (N knotpoints x batch)",
            "value": global_batch * args.steps / elapsed, "unit": "problem-sweeps/s", "n_gpus": chan.world,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": elapsed / args.steps * 1e3,
            "higher_is_better": True, "scaling": scaling, "vs_baseline": None, "dtype": "f64", "data": "synthetic",
            "config": {"workload": ("C3 bicycle tracking (BASELINE.json configs[3]), steering bound as an AL block"
                                    if c3 else "C2 pendulum swing-up (BASELINE.json configs[2])"),
                       "horizon_N": N, "n": n, "m": m, "batch_per_gpu": batch, "global_batch": global_batch,
                       "sharding": ("global batch %d split into contiguous per-rank ranges (strong scaling: rank 0 holds "
                                    "%d problems)" % (global_batch, batch)) if scaling == "strong" else
                                   ("%d problems per GPU x %d GPU(s) (weak scaling)" % (batch, chan.world)),
                       "plan": "LANE (lane-per-problem SoA)",
                       "kernels": {name_b: dict(kern[0], GBps=bytes_b / dur_b / 1e9),
                                   name_f: dict(kern[1], GBps=bytes_f / (ms_f / nf * 1e-3) / 1e9)},
                       "repeat": rep, "stats": stats, "full_solve": full_solve},
            "roofline": roofline_block("c3" if c3 else "c2", batch, N, name_b, bytes_b, dur_b),
            "roofline_forward": roofline_block("c3" if c3 else "c2", batch, N, name_f, bytes_f, ms_f / nf * 1e-3, slot=1),
        }))
    bt.close()
    chan.close()
    if world > 1:
        dist.destroy_process_group()


def ilqr_sweep_time(bt, torch, reps=5):
    """one iLQR sweep = expansion + BackwardPass + one forward evaluation with derivative (alpha = 1), i.e.
    CalcExpansions / BackwardPass / MeritFunction of solver.cpp:447-456, on the C1 batch (outside the timed region; host
    clock around the three C-ABI calls with the stream drained, median of `reps`)."""
    ts = {"expand": [], "backward": [], "merit": [], "total": []}
    for _ in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter(); bt.expand(); bt.synchronize()
        t1 = time.perf_counter(); bt.backward(); bt.synchronize()
        t2 = time.perf_counter(); bt.merit(1.0, derivative=True)
        t3 = time.perf_counter()
        for k, v in (("expand", t1 - t0), ("backward", t2 - t1), ("merit", t3 - t2), ("total", t3 - t0)):
            ts[k].append(v * 1e3)
    med = {k: sorted(v[1:])[len(v[1:]) // 2] for k, v in ts.items()}      # the first round is untimed
    return {"ms": med["total"], "expand_ms": med["expand"], "backward_ms": med["backward"],
            "merit_with_derivative_ms": med["merit"],
            "what": "altro_hip_expand + altro_hip_backward + altro_hip_merit(alpha = 1, phi and dphi): SURVEY 8(d)'s sweep "
                    "(expansion + BackwardPass + one forward evaluation with derivative), host clock, median of %d.  The expansion "
                    "launches nothing here: the merit pass with derivative leaves lx, lu of its candidate in the records and an "
                    "unconstrained quadratic cost's Hessian blocks are constants (round 4; before, a separate gradient pass re-read "
                    "the trajectory: 0.12-0.14 ms)" % reps}


DUMP_BYTES = 64 << 20    # --dump-outputs writes at most this much


def dump_outputs(bt, torch, out_dir, first, f32):
    """--dump-outputs DIR: what the last timed step (altro_hip_sweep) hands its caller -- delta_V and status of the whole batch,
    K, d, P, p, x, u, y of a fixed seeded sample of problems (their global indices: problems.npy) sized to keep all files under
    DUMP_BYTES.  The per-problem arrays are fetched in device-pointer mode and sampled on the device (P of the whole C1 batch alone
    is 1.2 GB).  float32 for an fp32 handle (the values it stores), float64 otherwise."""
    import ctypes
    N, n, m, B = bt.N, bt.n, bt.m, bt.batch
    dt = np.float32 if f32 else np.float64
    shapes = {"K": (N, m * n), "d": (N, m), "P": (N + 1, n * n), "p": (N + 1, n), "x": (N + 1, n), "u": (N, m), "y": (N + 1, n)}
    out = {"delta_V": bt.get("delta_V").astype(dt), "status": bt.get("status").astype(dt)}
    per_problem = sum(int(np.prod(s)) for s in shapes.values()) * np.dtype(dt).itemsize + 8
    count = max(1, min(B, 64, (DUMP_BYTES - sum(a.nbytes for a in out.values())) // per_problem))
    idx = np.sort(np.random.default_rng(20261016).choice(B, count, replace=False))
    out["problems"] = (first + idx).astype(np.float64)
    sel = torch.as_tensor(idx, device="cuda")
    bt.set_pointer_mode(True)
    try:
        for name, shp in shapes.items():
            buf = torch.empty((B,) + shp, dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            rc = getattr(bt.L, "altro_hip_get_" + name)(bt.h, ctypes.c_void_p(buf.data_ptr()))
            if rc != 0:
                raise RuntimeError("altro_hip_get_%s failed (%d): %s" % (name, rc, bt.L.altro_hip_last_error().decode()))
            out[name] = buf.index_select(0, sel).cpu().numpy().astype(dt)
            del buf
    finally:
        bt.set_pointer_mode(False)
        torch.cuda.empty_cache()
    os.makedirs(out_dir, exist_ok=True)
    for name, a in out.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)


_JSON_OUT = None


def _claim_stdout():
    """The contract: rank 0 prints ONE JSON line on stdout.  Native libraries write there too (RCCL prints a version
    banner on its first communicator), so fd 1 is pointed at stderr for the life of the process and the line goes to
    a private duplicate of the original stdout."""
    global _JSON_OUT
    sys.stdout.flush()
    _JSON_OUT = os.fdopen(os.dup(1), "w")
    os.dup2(2, 1)


def emit(obj):
    _JSON_OUT.write(json.dumps(obj) + "\n")
    _JSON_OUT.flush()


def main():
    args = parse()
    relaunch_if_needed(args)
    _claim_stdout()
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    # The CPU legs run first, before any HIP state exists in this process (the all-cores leg forks workers).
    cpu_leg = None
    if args.full and world == 1 and not args.no_cpu_baseline and args.config == "c1":
        cpu_leg = cpu_baseline(args.horizon, args.cpu_seconds)
        cpu_leg["all_cores"] = cpu_all_cores(args.horizon)
        cpu_leg["eigen"] = eigen_probe()
    # roofline.traffic of THIS run: two short PMC passes of the same command as child processes, before this process touches the
    # GPU (one GPU only: the driver's multi-GPU runs keep the tracked figure)
    global _LIVE_TRAFFIC, _LIVE_TRAFFIC_NOTE
    if args.full and not args.no_live_traffic and rank == 0 and world == 1:
        t_live = time.perf_counter()
        try:
            _LIVE_TRAFFIC = live_traffic(args)
            _LIVE_TRAFFIC_NOTE = ("measured in this run (%.0f s)" % (time.perf_counter() - t_live)) if _LIVE_TRAFFIC else \
                "the live PMC passes failed or rocprofv3 is absent: tracked figure"
        except Exception as e:   # noqa: BLE001 -- a measurement extra must never take the bench line down
            print("[bench] live traffic failed: %s" % e, file=sys.stderr)
            _LIVE_TRAFFIC_NOTE = "the live PMC passes failed (%s): tracked figure" % e
    else:
        _LIVE_TRAFFIC_NOTE = ("without --full: tracked figure" if not args.full else "--no-live-traffic" if args.no_live_traffic
                              else "more than one rank: tracked figure")
    # ... and of the other single-GPU configs the line carries (C2, C3 at 8192 and 65536, C4): the same two passes each
    live_other = {}
    if (args.full and not args.no_live_traffic and rank == 0 and world == 1 and args.config == "c1" and not args.no_other_configs
            and not args.sweeps_only):
        for key, (cfg_o, batch_o) in {"c2": ("c2", 8192), "c3_8192": ("c3", 8192), "c3_65536": ("c3", 65536), "c4": ("c4", 16384)}.items():
            try:
                live_other[key] = live_traffic(args, config=cfg_o, batch=batch_o)
            except Exception as e:   # noqa: BLE001
                print("[bench] live traffic of %s failed: %s" % (key, e), file=sys.stderr)
    seam = None
    if args.full and rank == 0 and world == 1 and args.config == "c1" and not args.sweeps_only and not args.no_cpu_baseline:
        seam = single_problem_seam()
    import torch
    import torch.distributed as dist
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the HIP hot path has no CPU fallback")
    # One rank per GPU.  (ALTRO_BENCH_BACKEND=gloo is a test hook: it lets a 1-GPU box execute the multi-rank code
    # path with every rank on GPU 0 and the scalar reductions on the CPU; the driver's runs use nccl == RCCL.)
    backend = os.environ.get("ALTRO_BENCH_BACKEND", "nccl")
    if backend != "nccl":
        local_rank = local_rank % torch.cuda.device_count()
    torch.cuda.set_device(local_rank)
    global RED_DEVICE
    RED_DEVICE = "cuda" if backend == "nccl" else "cpu"
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(backend, rank=rank, world_size=world)

    import altro_amd
    from altro_amd import shard
    from tests import problems
    if backend == "nccl" and torch.cuda.device_count() < world:
        raise SystemExit("bench.py: %d ranks but only %d HIP device(s) are visible" % (world, torch.cuda.device_count()))
    chan = StatsChannel(local_rank, rank, world, shard, dist)      # the RCCL communicator, opened before anything is timed
    if chan.world != args.gpus:
        raise SystemExit("bench.py: --gpus %d but the communicator has %d rank(s)" % (args.gpus, chan.world))
    # every rank says which communicator it actually joined, BEFORE anything is timed (stderr: stdout carries the one JSON line)
    print("[bench] rank %d / %d on device %d (%s): statistics channel = %s" % (rank, world, local_rank,
          torch.cuda.get_device_properties(local_rank).name, chan.how), file=sys.stderr, flush=True)
    N, n, m = args.horizon, 12, 4
    c4 = args.config == "c4"
    args.c4_pure = c4 and not args.c4_mixed
    if c4:
        N = 512 if args.horizon == 256 else args.horizon
    if args.config in ("c2", "c3"):
        return lane_config(args, rank, local_rank, world, dist, torch, chan)
    batch, first, global_batch, scaling = resolve_batch(args, 16384 if c4 else 4096, rank, world)
    bt = make_mfma_batch(c4, args.c4_pure, batch, first, N, local_rank)

    elapsed, kern = timed_region(bt, args, world, dist, torch, shard)
    if args.dump_outputs and rank == 0:
        dump_outputs(bt, torch, args.dump_outputs, first, c4)
    rep = repeat_block(bt, torch, elapsed / args.steps * 1e3, args.repeat_seconds if args.full else 0)
    ms_b, nb, name_b = kern[0]["avg_ms"], 1, kern[0]["name"]
    ms_f, nf, name_f = kern[1]["avg_ms"], 1, kern[1]["name"]

    # the same batch as a full iLQR solve (rollout, expansion, backward sweep, merit-function line search,
    # convergence test; an LQ problem, so <= 3 sweeps), outside the timed region
    # who ran what: one row per rank (device, PCI bus id, its own K-step time) so that a straggler or a mis-bound rank shows
    ranks = rank_table(elapsed_local(), args.steps, local_rank, rank, world, dist, torch) if args.full else None
    full_solve, ilqr_sweep = None, None
    if args.full and not c4 and not args.sweeps_only:
        Qd2 = np.stack([np.ones(n), 100.0 * np.ones(n)])
        bt.set_tracking_cost(Qd2, np.full((1, m), 1e-2), np.zeros((2, n)), np.zeros((1, m)), k_stride_zero=True,
                             batch_stride_zero=True)
        for timed in (False, True):   # one untimed solve first: the first launch of each kernel loads its code object
            bt.set_input_guess(np.zeros((1, 1, m)), k_stride_zero=True, batch_stride_zero=True)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            res = bt.ilqr_solve(iterations_max=10)
            torch.cuda.synchronize()
            t_solve = time.perf_counter() - t1
        full_solve = {"seconds": t_solve, "sweeps": int(res["sweeps"]), "merit_launches": int(res["merit_launches"]),
                      "converged": int((res["status"] == 0).sum()), "problems_per_s": batch / t_solve}
        ilqr_sweep = ilqr_sweep_time(bt, torch)

    # solver statistics -- the only thing that ever crosses GPUs (RCCL over xGMI, latency-bound) -- after the solve,
    # so that the quantities SolverImpl::Solve reports are all populated (for c4: the sweep's quantities only)
    stats = chan.reduce(bt) if args.full else None

    # ... and, after the statistics (they describe the unconstrained solve), the same batch with input bounds |u| <= 2 as a whole
    # AL-iLQR solve: constraint rows, dual and penalty updates, line searches past the first step -- the AL half of the path
    # (SURVEY section 8 row f2), outside the timed region like the solve above
    constrained = None
    if args.full and not c4 and not args.sweeps_only:
        import altro_amd
        Gb = np.zeros((2 * m, n + m)); Gb[:m, n:] = np.eye(m); Gb[m:, n:] = -np.eye(m)
        bt.add_linear_constraint(0, N - 1, altro_amd.CONE_INEQUALITY, Gb, np.full(2 * m, 2.0))
        for timed in (False, True):
            bt.set_input_guess(np.zeros((1, 1, m)), k_stride_zero=True, batch_stride_zero=True)
            bt.reset_duals(1.0)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            resc = bt.ilqr_solve(iterations_max=40)
            torch.cuda.synchronize()
            t_con = time.perf_counter() - t1
        constrained = {"seconds": t_con, "sweeps": int(resc["sweeps"]), "merit_launches": int(resc["merit_launches"]),
                       "converged": int((resc["status"] == 0).sum()), "dual_updates_max": int(resc["dual_updates"].max()),
                       "max_feasibility": float(np.abs(resc["feasibility"]).max()),
                       "what": "the C1 batch with input bounds |u| <= 2 (an INEQUALITY block at every k < N) as one altro_hip_ilqr_solve: "
                               "AL-iLQR, cubic line search, iterations_max 40 (host clock, second of two solves)"}

    # the other single-GPU configs of BASELINE.json, each a short timed region of its own on this GPU (one-GPU runs of the
    # default config only; the C1 handle is released first: C4 alone holds 18 GB)
    others = None
    if args.full and not c4 and world == 1 and not args.no_other_configs and not args.sweeps_only:
        bytes_keep = (bt.algorithmic_bytes(0), bt.algorithmic_bytes(1))
        bt.close()
        bt = None
        others = {}
        for key in ("c2", "c3_8192", "c3_65536", "c4"):
            try:
                others[key] = other_config_entry(key, local_rank, args.other_steps, torch, 0.0 if args.no_cpu_baseline else 2.0,
                                                 live=live_other.get(key))
            except Exception as e:   # noqa: BLE001 -- an extra must never take the metric's own line down
                others[key] = {"error": str(e)}
        for (n_, m_) in ((13, 4), (28, 4)):   # plan MFMA32: the shapes one step past the tile (round 6)
            try:
                others["mfma32_%dx%d" % (n_, m_)] = mfma32_entry(n_, m_, local_rank, args.other_steps, torch, 0.0 if args.no_cpu_baseline else 2.0)
            except Exception as e:   # noqa: BLE001
                others["mfma32_%dx%d" % (n_, m_)] = {"error": str(e)}
        try:   # nonlinear dynamics past the tile: the device model in the row-layout loop kernels (round 6)
            others["quad13_nmpc"] = quad13_nmpc_entry(local_rank, torch)
        except Exception as e:   # noqa: BLE001
            others["quad13_nmpc"] = {"error": str(e)}
    else:
        bytes_keep = (bt.algorithmic_bytes(0), bt.algorithmic_bytes(1))

    if rank == 0:
        total_problems = global_batch
        sweeps_per_s = total_problems * args.steps / elapsed
        bytes_b, bytes_f = bytes_keep
        dur_b = ms_b / nb * 1e-3
        dur_f = ms_f / nf * 1e-3
        out = {
            "metric": "iLQR backward+forward sweeps/sec (N knotpoints x batch)",
            "value": sweeps_per_s,
            "unit": "problem-sweeps/s",
            "n_gpus": chan.world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3,
            "higher_is_better": True,
            "scaling": scaling,
            "vs_baseline": None,
            "dtype": ("f32" if args.c4_pure else "f32 storage, f64 tile arithmetic") if c4 else "f64",
            "data": "synthetic",
            "config": {
                "workload": ("C4 random LTV TVLQR sweep, fp32 storage (BASELINE.json configs[4])" if c4 else
                             "C1 double integrator TVLQR sweep (BASELINE.json configs[1])"),
                "horizon_N": N, "n": n, "m": m, "batch_per_gpu": batch, "global_batch": total_problems,
                "parallelism": "problem instances sharded over %d GPU(s), no data-path collective; "
                               "RCCL all-reduce of solver stats only" % chan.world,
                "sharding": ("global batch %d split into contiguous per-rank ranges (strong scaling)" % global_batch)
                            if scaling == "strong" else "%d problems per GPU x %d GPU(s) (weak scaling)" % (batch, chan.world),
                "plan": ("MFMA16, pure fp32: four problems per wave, v_mfma_f32_16x16x4 + v_mfma_f32_16x16x1_4b" if args.c4_pure else
                         "MFMA16 (wave-per-problem, v_mfma_f64_16x16x4)"),
                "knotpoint_steps_per_s": sweeps_per_s * N,
                "kernels": {name_b: dict(kern[0], algorithmic_GB=bytes_b / 1e9, GBps=bytes_b / dur_b / 1e9),
                            name_f: dict(kern[1], algorithmic_GB=bytes_f / 1e9, GBps=bytes_f / dur_f / 1e9)},
                "repeat": rep,
                "stats": stats,
                "ilqr_full_solve": full_solve,
                "ilqr_sweep": ilqr_sweep,
                "ilqr_constrained_solve": constrained,
                "ranks": ranks,
                "other_configs": others,
            },
            "roofline": roofline_block(("c4pure" if args.c4_pure else "c4mixed") if c4 else "c1", batch, N, name_b, bytes_b, dur_b),
            "roofline_forward": roofline_block(("c4pure" if args.c4_pure else "c4mixed") if c4 else "c1", batch, N, name_f,
                                               bytes_f, dur_f, slot=1),
        }
        if c4:
            out["config"]["c4_numerics"] = {
                "default": "pure fp32 (ALTRO_HIP_F32_PURE): fp32 records, fp32 MFMA arithmetic -- configs[4] says fp32" if args.c4_pure
                           else "fp32 records, fp64 tile arithmetic (the C ABI's ALTRO_HIP_F32 default)",
                "accuracy_vs_fp64_oracle": "K, d, P, p relative to the fp64 oracle on the same fp32-rounded inputs through all "
                                           "512 knot points: 2e-5 pure fp32, 5e-7 fp64 tile arithmetic "
                                           "(tests/test_gpu_parity.py::test_c4_full_horizon_sample_vs_oracle holds both)",
                "other_variant": "--c4-mixed" if args.c4_pure else "(default) pure fp32"}
        out["roofline"]["has_f"] = True
        out["roofline"]["has_f_note"] = "the batch carries the affine term f (zeros for C1): the HAS_F = true instantiation is timed, all 5088 B per knot point of SURVEY 8(d) are read or written"
        # the two fractions side by side at top level: algorithmic bytes (the contract's `frac`) and the bytes that physically moved
        out["frac_algorithmic"] = out["roofline"]["frac"]
        out["frac_traffic"] = out["roofline"]["frac_traffic"]
        out["roofline"]["traffic_live"] = _LIVE_TRAFFIC_NOTE
        if ilqr_sweep is not None:
            # one sweep = expansion + BackwardPass + one forward evaluation with derivative; its algorithmic bytes per knot
            # point = backward (3n^2+3nm+m^2+3n+2m) + nonlinear forward (2n^2+2nm+5n+4m: K, d, P, p, nominal x, u in; x_, u_, y_, A, B, lx, lu out)
            el = (3 * n * n + 3 * n * m + m * m + 3 * n + 2 * m) + (2 * n * n + 2 * n * m + 5 * n + 4 * m)
            sweep_bytes = el * 8.0 * N * batch
            ach = sweep_bytes / (ilqr_sweep["ms"] * 1e-3) / 1e9
            out["ilqr_sweep"] = dict(ilqr_sweep, value=batch / (ilqr_sweep["ms"] * 1e-3), unit="problem-sweeps/s (per GPU)",
                                     roofline={"bound": "hbm", "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": ach / HBM_PEAK_GBS,
                                               "algorithmic_bytes_per_knot_point": el * 8,
                                               "note": "whole-sweep fraction on the host clock (three C-ABI calls, stream drained between them): "
                                                       "(636 + 460) elements x 8 B x N x batch / time / 8 TB/s"})
        if seam is not None:
            out["single_problem_seam"] = seam
        if cpu_leg is not None:
            out["cpu_baseline"] = cpu_leg
        emit(out)
    if bt is not None:
        bt.close()
    chan.close()
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
