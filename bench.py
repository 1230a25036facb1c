#!/usr/bin/env python3
"""Flagship benchmark: RAFT-Stereo sceneflow 480x640 (32 GRU iterations) throughput on N MI355X.

Contract (driver): ``python bench.py --gpus N --steps K --warmup W``.  N > 1 works two ways:

* under ``torch.distributed.run`` (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* set by the launcher):
  ``--gpus`` must equal WORLD_SIZE, otherwise the run fails loudly;
* directly (``python bench.py --gpus 8``): the parent process — which never touches the GPU — spawns N
  fresh rank processes with RANK / LOCAL_RANK / WORLD_SIZE / MASTER_ADDR=127.0.0.1 / MASTER_PORT set,
  forwards their output and exits with the first failing rank's code.

Under RCCL (backend ``nccl``) rank r owns GPU LOCAL_RANK; asking for more ranks than visible GPUs exits
non-zero (no silent oversubscription).  ``SA_DIST_BACKEND=gloo`` is the rehearsal mode (ranks may share a
GPU, or run on the CPU with ``--device cpu``, which swaps the native engine for the PyTorch oracle so
the launcher / sharding / gather plumbing is testable without a GPU — that mode is labelled in the JSON
and is never a performance number).

One step = every rank runs its shard of stereo pairs (``--per-gpu-batch``, default 8 => 64 pairs on 8 GPUs,
BASELINE.json config 5) through the native engine (one hipGraph per frame batch: preprocess, encoders, corr
pyramid, 32 ConvGRU iterations, convex upsample), fed by an H2D copy of the inputs from pinned host memory
(copy stream, double-buffered, overlapping the previous step), then an RCCL all-gather of the disparity maps
over xGMI (issued async on the process group's stream, so step t's gather overlaps step t+1's frame graph).
K steps are timed between barrier + device synchronize; rank 0 prints ONE JSON line with the whole-job FPS
(max time over ranks).  Data: synthetic stereo pairs; weights: seeded random init of the upstream
architecture.

A plain run does only that: set up, warm up, time the K steps, print the line (rank 0 extra fields: the rank ->
device map, the engine's device footprint, the tactic plan).  ``--full`` adds the measurements that take runs of
their own: the all-gather alone (ms per step, measured after the timed region) and — single-process runs only,
unless ``--no-latency`` — batch-1 latency in the reference's timed region (pinned copy, H2D, network,
reprojection, D2H of disparity + point cloud; RAFTStereo/src/TRTRAFTStereo.cpp:119-146) for every model preset.

``--dump-outputs DIR`` (rank 0) writes what the last timed step returned to its caller as float32 ``.npy`` files:
``DIR/disparity.npy`` (the gathered disparity maps, [world * B, H, W]) and the rank's point cloud, whole as
``DIR/cloud.npy`` ([B, H, W, 6]) when its share of DUMP_BUDGET bytes covers it, otherwise (the default 8 x 480 x
640) ``DIR/cloud_sample.npy`` ([n, 6]: the pixels ``dump_sample_index`` picks, a fixed seeded choice in ascending
pixel order; ``dump_outputs`` has the rule, the result line's ``dumped_outputs`` names what was written).  Inputs
and weights are seeded, so two builds run with the same arguments can be compared output for output.

The engine normally times every conv shape's tactics when it is built, and two runs whose noisy timings pick
different tactics differ in the last bits of the disparity (and, where the disparity is near zero, by any amount in
the reprojected cloud).  For the workloads with a plan under ``bench_plans/`` (the default one) bench.py therefore
pins that committed plan instead: every run launches the same kernels and writes the same outputs, and nothing is
tuned (``plan_source`` in the result line).  ``--tune`` restores the tuner; ``--export-plan FILE`` writes the plan
the engine launched, which is how a committed plan is refreshed after the tactics change.
"""
from __future__ import annotations

import argparse
import gc
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stereoalgorithms_amd  # noqa: E402,F401  (HIP runtime env defaults before torch touches the GPU)

BASELINE_MS = {"raftstereo-sceneflow": 38.0, "raftstereo-realtime": 11.0}  # RTX 3090, README_en.md:139-141
# the other model families' published RTX 3090 numbers (README_en.md:192-194,244-246,293-295)
OTHER_MS = {"crestereo-iter2": 12.0, "crestereo-iter5": 23.0, "crestereo-iter10": 42.0, "hitnet-d400": 15.0,
            "hitnet-xl": None, "fastacvnet-plus": 12.0}  # flyingthings_finalpass_xl: no published latency
ITERS = {"raftstereo-sceneflow": 32, "raftstereo-realtime": 7}


def parse(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--model", default="raftstereo-sceneflow")
    p.add_argument("--per-gpu-batch", type=int, default=8)
    p.add_argument("--height", type=int, default=480)
    p.add_argument("--width", type=int, default=640)
    p.add_argument("--iters", type=int, default=-1, help="override GRU iterations (tests only)")
    p.add_argument("--latency-frames", type=int, default=20)
    p.add_argument("--no-latency", action="store_true", help="with --full: skip the batch-1 latency block")
    p.add_argument("--full", action="store_true",
                   help="also measure what the headline does not need: the all-gather alone, batch-1 latency per preset")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="write the last timed step's outputs as DIR/<name>.npy (float32, DUMP_BUDGET bytes at most)")
    p.add_argument("--tune", action="store_true",
                   help="time the conv tactics on this GPU instead of pinning the committed plan of the workload")
    p.add_argument("--export-plan", metavar="FILE", default=None,
                   help="write the tactic plan the engine launched (rank 0), e.g. to refresh bench_plans/")
    p.add_argument("--device", choices=("gpu", "cpu"), default="gpu",
                   help="cpu = PyTorch-oracle rehearsal of the launcher/DP plumbing (gloo only, not a benchmark)")
    args = p.parse_args(argv)
    if args.steps < 1 or args.warmup < 0:
        p.error("--steps must be at least 1 and --warmup at least 0")
    return args


PLAN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "bench_plans")


def committed_plan_path(args, arch: str = "gfx950") -> str | None:
    """The committed tactic plan of this workload (model, per-GPU batch, size; default iterations only), if any."""
    if args.iters > 0:
        return None
    path = os.path.join(PLAN_DIR, f"{args.model}_b{args.per_gpu_batch}_{args.height}x{args.width}_{arch}.plan")
    return path if os.path.exists(path) else None


def pin_committed_plan(path: str) -> int:
    """Load the entries of a committed plan into the process's tactic table and pin them, so the engine built next
    launches exactly these tactics whatever its tuner would measure and whatever plan file its cache holds: the
    outputs are then the same in every run.  A shape the file lacks is still tuned.  Plan files carry the id of the
    library build that timed them and the loader takes nothing from another build's; the committed entries name
    tactics by number only, so they are handed over under this build's id.  Returns the entries loaded."""
    import tempfile
    from stereoalgorithms_amd import _native as N
    lib = N.require_native()
    with open(path) as f:
        entries = [l for l in f if l.strip() and not l.startswith("#")]
    fd, tmp = tempfile.mkstemp(suffix=".plan")
    try:
        with os.fdopen(fd, "w") as f:
            f.write(f"# sa-plan build={lib.sa_plan_build_id().decode()}\n")
            f.writelines(entries)
        n = int(lib.sa_conv_plan_load(tmp.encode()))
    finally:
        os.unlink(tmp)
    if n != len(entries):
        raise RuntimeError(f"{path}: {n} of {len(entries)} plan entries accepted (tactic numbers of another build?)")
    lib.sa_conv_plan_pin(1)
    return n


DUMP_BUDGET = 60_000_000  # bytes of array data --dump-outputs writes at most, over all files


def dump_sample_index(n_rows: int, keep: int, seed: int = 0) -> np.ndarray:
    """The ``keep`` of ``n_rows`` rows a sampled dump holds: a seeded choice without replacement, ascending, so it is
    the same for every run and build."""
    return np.sort(np.random.default_rng(seed).choice(n_rows, size=keep, replace=False))


def dump_outputs(out_dir: str, arrays: dict) -> dict:
    """Write ``arrays`` (name -> (float32 ndarray, row width in elements)) under ``out_dir``.  Every array whose
    share of DUMP_BUDGET (what is left, split evenly over the arrays still to write) covers it is written whole as
    ``<name>.npy``; a larger one as ``<name>_sample.npy`` holding the rows dump_sample_index picks.  Returns
    name -> {file, shape, sampled_rows} for the result line."""
    os.makedirs(out_dir, exist_ok=True)
    left, todo, written = DUMP_BUDGET, len(arrays), {}
    for name, (a, width) in arrays.items():
        a = np.ascontiguousarray(a, dtype=np.float32)
        share, todo = left // todo, todo - 1
        fname, sampled = f"{name}.npy", None
        if a.nbytes > share:
            rows = a.reshape(-1, width)
            sampled = int(share // (width * 4))
            a = rows[dump_sample_index(rows.shape[0], sampled)]
            a = a.reshape(-1) if width == 1 else a
            fname = f"{name}_sample.npy"
        np.save(os.path.join(out_dir, fname), a)
        left -= a.nbytes
        written[name] = {"file": fname, "shape": list(a.shape), "sampled_rows": sampled}
    return written


def _free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def visible_gpus() -> int | None:
    """GPUs this process may use, counted without touching HIP: the KFD topology in sysfs (nodes with a GFX target),
    narrowed by HIP_VISIBLE_DEVICES / ROCR_VISIBLE_DEVICES / CUDA_VISIBLE_DEVICES.  None when sysfs is unreadable."""
    root = "/sys/class/kfd/kfd/topology/nodes"
    try:
        n = 0
        for d in os.listdir(root):
            try:
                props = open(os.path.join(root, d, "properties")).read().split()
            except OSError:
                continue
            kv = dict(zip(props[0::2], props[1::2]))
            if int(kv.get("gfx_target_version", "0")) != 0:
                n += 1
    except OSError:
        return None
    for var in ("ROCR_VISIBLE_DEVICES", "HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        v = os.environ.get(var)
        if v is not None:
            n = min(n, len([x for x in v.split(",") if x.strip() != ""]))
    return n


def launch(args, argv) -> int:
    """Parent of a self-launched N-rank job: spawn, forward output, propagate failure.

    The parent never initialises HIP (no torch.cuda call: on ROCm torch without amdsmi even device_count() would),
    so the children are fresh processes, never a fork / exec of a GPU-initialised one.  GPUs are counted from sysfs;
    each child re-checks LOCAL_RANK against its own device count."""
    n = args.gpus
    backend = os.environ.get("SA_DIST_BACKEND", "nccl")
    torch_mod = sys.modules.get("torch")
    assert torch_mod is None or not torch_mod.cuda.is_initialized(), "bench.py launcher: GPU initialised before spawn"
    if backend == "nccl" and args.device == "gpu":
        ndev = visible_gpus()
        if ndev is not None and n > ndev:
            print(f"bench.py: --gpus {n} but only {ndev} GPU(s) visible; RCCL needs one GPU per rank "
                  f"(SA_DIST_BACKEND=gloo to rehearse more ranks)", file=sys.stderr, flush=True)
            return 2
    port = int(os.environ.get("MASTER_PORT") or _free_port())
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR=os.environ.get("MASTER_ADDR", "127.0.0.1"), MASTER_PORT=str(port),
                   SA_BENCH_CHILD="1")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__), *argv], env=env))
    rc = 0
    alive = list(procs)
    while alive:
        for p in list(alive):
            code = p.poll()
            if code is None:
                continue
            alive.remove(p)
            if code != 0 and rc == 0:
                rc = code if code > 0 else 1
                for q in alive:  # one rank failed: the collectives of the others can never complete
                    q.terminate()
        time.sleep(0.05)
    for p in procs:
        p.wait()
    return rc


class OracleEngine:
    """CPU stand-in with the native engine's ``run`` contract (u8 BGR [B,H,W,3] -> disparity [B,H,W]),
    backed by the fp32 PyTorch oracle.  Used only by ``--device cpu`` rehearsals of the launcher."""

    def __init__(self, preset, h, w, batch, iters, seed=0):
        from stereoalgorithms_amd.models import raft_stereo as R
        self.model = R.build(preset, seed)
        self.batch, self.height, self.width = batch, h, w
        self.iters = iters if iters > 0 else R.PRESETS[preset].valid_iters
        self.device_bytes = 0

    def set_Q(self, Q):
        self.Q = Q

    def run(self, left, right, out=None, cloud=False, cloud_out=None):
        import torch
        with torch.no_grad():
            l = left.flip(-1).permute(0, 3, 1, 2).float()
            r = right.flip(-1).permute(0, 3, 1, 2).float()
            _, up = self.model(l, r, iters=self.iters)
            d = -up[:, 0]
        d = out.copy_(d) if out is not None else d.contiguous()
        if not cloud:
            return d
        from stereoalgorithms_amd.utils.geometry import reproject_cloud_torch
        c = reproject_cloud_torch(d, left, self.Q)
        return d, (cloud_out.copy_(c) if cloud_out is not None else c)


def main(argv=None) -> int:
    argv = list(sys.argv[1:] if argv is None else argv)
    args = parse(argv)
    env_world = os.environ.get("WORLD_SIZE")
    if env_world is None and args.gpus > 1:
        return launch(args, argv)
    world = int(env_world or "1")
    if world != args.gpus:
        print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}; launch one rank per requested GPU",
              file=sys.stderr, flush=True)
        return 2
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    backend = os.environ.get("SA_DIST_BACKEND", "nccl")  # nccl = RCCL over xGMI
    cpu = args.device == "cpu"
    if cpu and world > 1 and backend != "gloo":
        print("bench.py: --device cpu needs SA_DIST_BACKEND=gloo", file=sys.stderr, flush=True)
        return 2

    import torch
    import torch.distributed as dist

    if cpu:
        dev = torch.device("cpu")
        torch.set_num_threads(max(1, (os.cpu_count() or 1) // world))
    else:
        ndev = torch.cuda.device_count()
        if backend == "nccl" and local >= ndev:
            print(f"bench.py: rank {rank} has LOCAL_RANK {local} but only {ndev} GPU(s) are visible",
                  file=sys.stderr, flush=True)
            return 2
        # gloo rehearsal only: more ranks than GPUs share devices round-robin
        local_dev = local if backend == "nccl" else local % max(1, ndev)
        torch.cuda.set_device(local_dev)
        dev = torch.device("cuda", local_dev)
    # SA_DP_GATHER_WORLD1=1: a world-1 RCCL process group that still runs every step's all-gather, so the
    # H2D-copy / all-gather / frame-graph overlap of the multi-GPU path can be traced on one GPU
    force_gather = world == 1 and os.environ.get("SA_DP_GATHER_WORLD1") == "1" and not cpu
    if force_gather:
        os.environ.setdefault("MASTER_PORT", str(_free_port()))
    if world > 1 or force_gather:
        from datetime import timedelta
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        # bounded collectives: a rank that dies or hangs fails the job instead of stalling it
        kw = dict(device_id=dev) if (backend == "nccl" and not cpu) else {}
        dist.init_process_group(backend, rank=rank, world_size=world,
                                timeout=timedelta(seconds=int(os.environ.get("SA_DIST_TIMEOUT", "600"))), **kw)
        assert dist.get_world_size() == world and dist.get_rank() == rank

    from stereoalgorithms_amd.parallel.dp import DataParallelStereo, H2DPrefetcher, build_engine_shared_plan
    from stereoalgorithms_amd.utils.synthetic import batch_pairs

    B, H, W = args.per_gpu_batch, args.height, args.width
    Q = np.array([[1, 0, 0, -W / 2], [0, 1, 0, -H / 2], [0, 0, 0, 500.0], [0, 0, 1 / 60.0, 0]], np.float32)
    plan_digests = plan_file = plan_pinned = None
    if cpu:
        eng = OracleEngine(args.model, H, W, B, args.iters, seed=0)
        eng.set_Q(Q)
    else:
        from stereoalgorithms_amd.models.engine import NativeStereoEngine
        # every rank runs rank 0's tactic plan (rank 0 tunes, the others build from its broadcast plan bytes), so
        # no rank's noisy timing picks a slower kernel that would set the job's step time
        # the workload's committed plan, pinned on every rank (--tune: this GPU's own timings decide instead, and two
        # runs may then launch different tactics and differ in the last bits of their outputs)
        plan_file = None if args.tune else committed_plan_path(args)
        plan_pinned = pin_committed_plan(plan_file) if plan_file else None
        try:
            eng, plan_digests = build_engine_shared_plan(
                lambda: NativeStereoEngine(args.model, None, H, W, batch=B, iters=args.iters, device=dev.index, seed=0),
                world if (world > 1 or force_gather) else 1, rank)
        finally:
            if plan_file:
                from stereoalgorithms_amd import _native as N
                N.require_native().sa_conv_plan_pin(0)
        eng.set_Q(Q)
        if args.export_plan and rank == 0:
            err = eng.plan_export(args.export_plan)
            if err:
                raise OSError(err, f"could not write {args.export_plan}")
    # every rank reprojects its frames' point clouds in the frame graph and keeps them (the reference produces a
    # cloud per frame inside its timed region, RAFTStereo/src/TRTRAFTStereo.cpp:140-144)
    dp = DataParallelStereo(eng, world_size=world, rank=rank, force_gather=force_gather, cloud=True)
    l_np, r_np = batch_pairs(B, H, W, seed=100 * rank)
    left_h, right_h = torch.from_numpy(l_np), torch.from_numpy(r_np)
    if cpu:
        def step():
            return dp.step_async(left_h, right_h)

        def sync():
            pass
    else:
        left_h, right_h = left_h.pin_memory(), right_h.pin_memory()
        # Streams per rank: the engine's own stream is made torch's current stream, so frames launch there without a
        # cross-stream event pair and the step adds no caller stream; the H2D prefetch rides the engine's copy
        # stream (idle outside capture); RCCL's all-gather runs on the process group's stream.  That is 3 streams
        # (plus whatever the graph runtime uses for the frame graph's parallel branches) within GPU_MAX_HW_QUEUES=4.
        torch.cuda.set_stream(eng.main_stream)
        h2d = H2DPrefetcher([left_h, right_h], dev, stream=eng.copy_stream)

        h2d.prefetch([left_h, right_h])

        def step():
            # every step copies its inputs H2D on the copy stream, issued one step ahead (the copies of step t+1
            # are enqueued before step t, so they run under step t's frame graph, see H2DPrefetcher); the
            # all-gather of step t (RCCL's own stream) overlaps step t+1's frame graph
            h2d.prefetch([left_h, right_h])
            left, right = h2d.next()
            return dp.step_async(left, right)

        def sync():
            torch.cuda.synchronize()

    for _ in range(args.warmup):
        step()
    dp.flush()
    sync()
    if world > 1:
        dist.barrier()
    sync()
    t0 = time.perf_counter()
    pending = None
    for _ in range(args.steps):
        pending = step()
    out = pending.wait()
    cloud = pending.cloud
    dp.flush()  # every step's collective is complete inside the timed region
    sync()
    if world > 1:
        dist.barrier()
    sync()
    dt = time.perf_counter() - t0
    gather_ms = None
    ranks = [{"rank": rank, "device": str(dev), "host": socket.gethostname(),
              "plan_tactics": None if plan_digests is None else plan_digests[min(rank, len(plan_digests) - 1)],
              "step_ms": round(dt / args.steps * 1e3, 3)}]
    rank_ms = [dt / args.steps * 1e3]
    if world > 1:
        # every rank's own time (imbalance shows on the first real multi-GPU curve), then the job's = the slowest
        t = torch.tensor([dt], device=dev, dtype=torch.float64)
        ts_all = [torch.zeros_like(t) for _ in range(world)]
        dist.all_gather(ts_all, t)
        rank_ms = [x.item() / args.steps * 1e3 for x in ts_all]
        dt = max(x.item() for x in ts_all)
        gathered = [None] * world
        dist.all_gather_object(gathered, ranks[0])
        ranks = gathered
    assert out.shape == (world * B, H, W) and torch.isfinite(out).all()
    assert cloud is not None and cloud.shape == (B, H, W, 6)
    dumped = None
    if args.dump_outputs and rank == 0:
        # the tensors the last timed step handed back (gathered disparity, this rank's clouds), before anything else
        # runs on the engine
        dumped = dump_outputs(args.dump_outputs, {"disparity": (out.cpu().numpy(), 1), "cloud": (cloud.cpu().numpy(), 6)})
    if world > 1 and args.full:
        # the all-gather alone, outside the timed region (same message as one step's gather)
        send = out.new_empty((B, H, W))
        recv = out.new_empty((world * B, H, W))
        from stereoalgorithms_amd.parallel.dp import all_gather_disparity
        for _ in range(2):
            all_gather_disparity(send, world, recv)
        sync()
        dist.barrier()
        reps = 10
        tg = time.perf_counter()
        for _ in range(reps):
            all_gather_disparity(send, world, recv)
        sync()
        g = torch.tensor([(time.perf_counter() - tg) / reps * 1e3], device=dev, dtype=torch.float64)
        dist.all_reduce(g, op=dist.ReduceOp.MAX)
        gather_ms = round(g.item(), 4)

    ms_step = dt / args.steps * 1e3
    fps = world * B * args.steps / dt
    extra = {}
    # batch-1 latency block: single-process GPU runs only (in a multi-rank job the other ranks would sit in
    # process-group teardown while rank 0 builds and tunes more engines)
    plan_b8 = None if cpu else eng.plan_status
    dev_bytes_b8 = eng.device_bytes

    def release_step():
        """Tear the throughput step down in dependency order: the prefetcher's copies ride the engine's side stream,
        and torch's pinned-host allocator records an event on every stream that used a pinned block when that block
        is FREED -- so the pinned inputs, the prefetcher's buffers and events must go before the engine (and with it
        that stream) is destroyed.  Left to interpreter shutdown, the pinned blocks are freed after the stream is
        gone and the event record segfaults the exit."""
        nonlocal eng, dp, h2d, left_h, right_h
        sync()
        dp, h2d, left_h, right_h = None, None, None, None
        gc.collect()
        sync()
        if not cpu:
            torch.cuda.set_stream(torch.cuda.default_stream(dev))
            eng.close()
        eng = None

    h2d = None if cpu else h2d
    if rank == 0 and world == 1 and args.full and not args.no_latency and not cpu:
        release_step()
        import tempfile
        from stereoalgorithms_amd.models.engine import NativeStereoEngine
        wdir = tempfile.TemporaryDirectory()

        def weights_for(preset):
            """HITNet is timed on the scaled-init graph its 480x640 parity test validates (tests/test_hitnet_gpu.py):
            at the default init its coarse features are fp16-subnormal.  Same architecture and FLOPs either way."""
            if not preset.startswith("hitnet"):
                return None
            from stereoalgorithms_amd.models import hitnet as HN
            from stereoalgorithms_amd.utils.weights import save_model
            return str(save_model(HN.scale_init(HN.build(preset, seed=0)), os.path.join(wdir.name, f"{preset}.safetensors"),
                                  preset))

        for preset in ("raftstereo-sceneflow", "raftstereo-realtime", *OTHER_MS):
            # timed engine without stage stamps (they add serialising nodes to the frame graph)
            os.environ.pop("SA_STAGE_TIMES", None)
            wpath = weights_for(preset)
            e1 = NativeStereoEngine(preset if wpath is None else "", wpath, H, W, batch=1, device=dev.index, seed=0)
            e1.set_Q(Q)
            l1, r1 = l_np[:1].copy(), r_np[:1].copy()
            # caller-owned outputs allocated once outside the timed loop, as the reference's demo allocates its
            # point cloud (RAFTStereo/test/main.cpp:20); the timed region still copies both out every frame
            d_out = np.empty((1, H, W), np.float32)
            c_out = np.empty((1, H, W, 6), np.float32)
            for _ in range(3):
                e1.run_host(l1, r1, cloud=True, out=d_out, cloud_out=c_out)
            ts = []
            for _ in range(args.latency_frames):
                t1 = time.perf_counter()
                e1.run_host(l1, r1, cloud=True, out=d_out, cloud_out=c_out)
                ts.append((time.perf_counter() - t1) * 1e3)
            ts = np.array(ts)
            host_split = e1.host_times()  # last frame: input copies / enqueue / device wait + output copies
            # same timed region with the engine's pinned I/O buffers (host_buffers(): the camera writes its frame
            # there, the caller reads disparity + cloud there): H2D from pinned memory, and the frame graph's
            # reprojection writes both outputs to host memory itself, so no D2H copy and no pageable staging
            hb = e1.host_buffers()
            hb["left"][...] = l1
            hb["right"][...] = r1
            for _ in range(3):
                e1.run_host(hb["left"], hb["right"], cloud=True, out=hb["disp"], cloud_out=hb["cloud"])
            tp = []
            for _ in range(args.latency_frames):
                t1 = time.perf_counter()
                e1.run_host(hb["left"], hb["right"], cloud=True, out=hb["disp"], cloud_out=hb["cloud"])
                tp.append((time.perf_counter() - t1) * 1e3)
            tp = np.array(tp)
            pinned_ok = bool(np.array_equal(hb["disp"], d_out) and np.array_equal(hb["cloud"], c_out, equal_nan=True))
            hb = None
            dev_b1 = e1.device_bytes
            e1.close()
            # per-stage device times from a second engine with stamps in its graph (tactic plan cached)
            os.environ["SA_STAGE_TIMES"] = "1"
            e1 = NativeStereoEngine(preset if wpath is None else "", wpath, H, W, batch=1, device=dev.index, seed=0)
            e1.set_Q(Q)
            for _ in range(2):
                e1.run_host(l1, r1, cloud=True)
            base = {**BASELINE_MS, **OTHER_MS}[preset]
            extra[preset] = {"latency_ms_mean": round(float(ts.mean()), 3),
                             "latency_ms_p50": round(float(np.median(ts)), 3),
                             "latency_ms_p99": round(float(np.percentile(ts, 99)), 3),
                             "fps_b1": round(1000.0 / float(ts.mean()), 2),
                             "baseline_ms_rtx3090": base,
                             "speedup_vs_baseline": round(base / float(ts.mean()), 3) if base else None,
                             "latency_ms_pinned_io_mean": round(float(tp.mean()), 3),
                             "latency_ms_pinned_io_p99": round(float(np.percentile(tp, 99)), 3),
                             "pinned_io_matches": pinned_ok,
                             "device_bytes": dev_b1,
                             "host_split_ms_last_frame": host_split,
                             "weights": "scale_init (parity-tested graph)" if wpath else "seeded default init",
                             "plan_loaded": e1.plan_status["loaded"], "plan_state": e1.plan_status["state"],
                             "plan_saved": e1.plan_status["saved"], "plan_tactics": e1.plan_status["tactics"],
                             "device_stages_ms": {k: round(v, 3) for k, v in e1.stage_times()}}
            e1.close()
    if eng is not None:
        release_step()
    if rank == 0:
        base_fps = 1000.0 / BASELINE_MS[args.model]
        lat = extra.get(args.model, {}).get("latency_ms_mean")
        rec = {
            "metric": f"{args.model} {H}x{W} throughput (frames/s, whole job)",
            "value": round(fps, 3),
            "unit": "frames/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_step, 3),
            "higher_is_better": True,
            "scaling": "weak",
            # throughput (per-GPU batch B) over the reference's batch-1 FPS (1000 / 38 ms); the like-for-like
            # latency ratio is vs_baseline_latency_b1 (reference ms / our batch-1 ms in its timed region)
            "vs_baseline": round(fps / base_fps, 3),
            "vs_baseline_kind": "whole-job throughput vs reference batch-1 FPS (1000/ms)",
            "vs_baseline_latency_b1": round(BASELINE_MS[args.model] / lat, 3) if lat else None,
            "dtype": "fp32" if cpu else "fp16",
            "data": "synthetic stereo pairs, seeded random-init weights",
            "engine": "pytorch-oracle-cpu (plumbing rehearsal, not a benchmark)" if cpu else "native-hip",
            "config": {"model": args.model, "global_batch": world * B, "per_gpu_batch": B,
                       "resolution": f"{H}x{W}", "seq_len": None, "parallelism": f"dp{world}",
                       "iters": args.iters if args.iters > 0 else ITERS.get(args.model)},
            "world_size": world,
            "backend": backend if world > 1 else None,
            "ranks": ranks,
            "step_latency_ms": round(ms_step, 3),
            "rank_step_ms": {"min": round(min(rank_ms), 3), "max": round(max(rank_ms), 3)},
            "ms_per_frame_per_gpu": round(ms_step / B, 3),
            "allgather_ms": gather_ms,
            "allgather_bytes_per_rank": B * H * W * 4,
            "point_clouds": f"per rank [{B},{H},{W},6] fp32 XYZRGB, reprojected in the frame graph, kept local",
            "plan": None if cpu else plan_b8,
            # where the tactics came from: the committed plan (file under bench_plans/, entries pinned) or the tuner
            "plan_source": None if cpu else ({"committed": os.path.basename(plan_file), "entries": plan_pinned}
                                             if plan_file else "tuned"),
            # launched-tactic digests of every rank (None = some rank could not report one: unknown, not "equal")
            "plans_identical_across_ranks": (None if plan_digests is None or None in plan_digests
                                             else len(set(plan_digests)) == 1),
            "device_bytes": dev_bytes_b8,
            "latency_b1": extra,
            "full": args.full,
            "dumped_outputs": dumped,
        }
        print(json.dumps(rec), flush=True)
    if world > 1 or force_gather:
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
