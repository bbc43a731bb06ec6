"""Distributed tier (CPU, Gloo, world sizes 2, 3 and 8): batch-DP inference with overlapped all-gather
equals the single-process result; bench.py harness under torch.distributed.run (including the
driver's 8-process launch line)."""
import os
import socket
import subprocess
import sys

import pytest
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, q, device="cpu", backend="rccl"):
    try:
        _worker_body(rank, world, port, q, device, backend)
    except BaseException as e:  # surface failures instead of a queue timeout
        q.put((rank, repr(e), None, None))
        raise


def _worker_body(rank, world, port, q, device="cpu", backend="rccl"):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    sys.path.insert(0, ROOT)
    import torch.distributed as dist

    from tensorrt_dft_plugins_amd.models import AFNOConfig, AFNONet
    from tensorrt_dft_plugins_amd.parallel import DataParallelInference, init_distributed

    init_distributed("gloo")
    torch.manual_seed(0)  # same weights on every rank
    cfg = AFNOConfig(img_size=(48, 96), in_chans=4, out_chans=4, embed_dim=64, depth=2, num_blocks=4)
    model = AFNONet(cfg, backend="amd").eval().to(device)
    g = torch.Generator().manual_seed(100 + rank)
    xs = [torch.randn(2, cfg.in_chans, *cfg.img_size, generator=g).to(device) for _ in range(3)]
    dp = DataParallelInference(model, xs[0], gather=True, use_graph=device != "cpu", gather_backend=backend)
    outs = []
    for k in range(3):  # a different input per step and rank: slot / ordering mix-ups show
        dp.inputs.copy_(xs[k])
        outs.append(dp.step())
    dp.drain()
    if device != "cpu":
        torch.cuda.synchronize()
    full = [outs[1].clone().cpu(), outs[2].clone().cpu()]  # slots of steps 1 and 2
    with torch.no_grad():
        local = [model(xs[1]).cpu(), model(xs[2]).cpu()]
    # the runner's own collective self-check (bench.py records it), then again after rank 0
    # corrupts one word of its gathered copy: every rank must report the mismatch
    ok = dp.verify_gather()
    if rank == 0:
        dp.full[dp.last_slot()].view(-1)[world * 7 % dp.full[dp.last_slot()].numel()] += 1.0
    bad = dp.verify_gather()
    dp.close()
    # numpy arrays pickle by value: a torch tensor would travel as a shared-memory handle that the
    # parent can only open while this process is still alive (ConnectionResetError races)
    q.put((rank, [t.numpy() for t in full], [t.numpy() for t in local], (ok, bad)))
    dist.barrier()
    dist.destroy_process_group()


def _run_dp(device, backend="rccl", world=2):
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q, device, backend)) for r in range(world)]
    for p in procs:
        p.start()
    res = {}
    for _ in range(world):
        r, full, local, check = q.get(timeout=300)
        assert local is not None, f"rank {r} failed: {full}"
        res[r] = (full, local)
        ok, bad = check
        assert ok == {"gather_verified": True, "gather_mismatches": 0}, (r, ok)
        assert bad["gather_verified"] is False and bad["gather_mismatches"] >= 1, (r, bad)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for step in (0, 1):
        expected = torch.cat([torch.from_numpy(res[r][1][step]) for r in range(world)], 0)
        for r in range(world):
            got = torch.from_numpy(res[r][0][step])
            assert got.shape == expected.shape
            assert torch.allclose(got, expected, atol=1e-5), (r, step)


@pytest.mark.parametrize("backend", ["rccl", "ipc"])
def test_dp_allgather_gloo_world2(backend):
    """CPU, Gloo, world 2: the RCCL-path collective (Gloo all_gather) and the direct-push IPC
    protocol (/dev/shm transport: same slot / offset / handshake logic as the GPU transport)."""
    _run_dp("cpu", backend)


@pytest.mark.parametrize("backend", ["rccl", "ipc"])
def test_dp_allgather_gloo_world3(backend):
    """An odd world size: every rank's slot offset and every peer push list differ from world 2."""
    _run_dp("cpu", backend, world=3)


@pytest.mark.parametrize("backend", ["rccl", "ipc"])
def test_dp_allgather_gloo_world8(backend):
    """The 8-GPU node's rank count, rehearsed on the CPU: 8 processes, every rank pushes into 7
    peers' buffers at 8 different slot offsets (ipc) or joins an 8-way all_gather (rccl path on
    Gloo), and every rank's gathered output equals the concatenation of the 8 local results."""
    _run_dp("cpu", backend, world=8)


def _slow_consumer_worker(rank, world, port, q, release, protocol="flags"):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
        sys.path.insert(0, ROOT)
        import time

        import torch.distributed as dist

        from tensorrt_dft_plugins_amd.parallel import IpcAllGather

        dist.init_process_group("gloo")
        g = IpcAllGather([4, 8], torch.float32, torch.device("cpu"), nbuf=2, release=release, protocol=protocol)
        barriers = [0]
        real_barrier = dist.barrier

        def counting_barrier(*a, **k):
            barriers[0] += 1
            return real_barrier(*a, **k)

        dist.barrier = counting_barrier  # host handshakes issued by the gathers below
        seen = []
        slow = rank == world - 1

        def consume(full):  # runs in this rank's stream order
            if slow:
                time.sleep(0.15)  # a lagging GPU: still reading its slot when peers run ahead
            seen.append(full.clone())

        prev = None
        for k in range(6):
            full = g.gather(torch.full((4, 8), float(100 * k + rank)), k)
            if prev is not None:  # pipelined consumer: step k-1's result is read after step k is enqueued
                g.enqueue(lambda t=prev: consume(t))
            prev = full
        g.enqueue(lambda t=prev: consume(t))
        n_barriers = barriers[0]
        dist.barrier = real_barrier
        g.synchronize()
        bad = [k for k, t in enumerate(seen)
               if not torch.equal(t.view(world, 4, 8)[:, 0, 0], torch.arange(world, dtype=torch.float32) + 100 * k)]
        g.close()
        q.put((rank, (bad, n_barriers)))
        dist.destroy_process_group()
    except BaseException as e:
        q.put((rank, repr(e)))
        raise


def _run_slow_consumer(world, release, protocol="flags"):
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_slow_consumer_worker, args=(r, world, port, q, release, protocol))
             for r in range(world)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=300) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
    for r, v in res.items():
        assert isinstance(v, tuple), f"rank {r} failed: {v}"
    return res


@pytest.mark.parametrize("world,protocol", [(2, "flags"), (3, "flags"), (8, "flags"), (2, "events"), (3, "events")])
def test_ipc_gather_slow_consumer_slot_reuse(world, protocol):
    """Write-after-read across processes: every rank reads step k's gathered slot after it has
    enqueued step k + 1 (the overlap the double buffer is for); the last rank's stream lags (each
    read sleeps) while the others race ahead and reuse the slot at step k + 2.  The release step
    (parallel/ipc_gather.py: counted flags, or events + host barriers) makes every push wait until
    the slow rank has read the slot's previous contents: every rank sees every step intact.  The
    flags protocol does it without a single host barrier on the gather path."""
    res = _run_slow_consumer(world, release=True, protocol=protocol)
    assert all(v[0] == [] for v in res.values()), res
    if protocol == "flags":
        assert all(v[1] == 0 for v in res.values()), res
    else:
        assert all(v[1] == 2 * 6 for v in res.values()), res


@pytest.mark.parametrize("protocol", ["flags", "events"])
def test_ipc_gather_slow_consumer_detects_race_without_release(protocol):
    """The same run with the release wait disabled corrupts the slow rank's reads: the test above
    can see the race it guards against."""
    res = _run_slow_consumer(2, release=False, protocol=protocol)
    assert res[1][0], "expected the lagging rank to read overwritten slots"


@pytest.mark.gpu
@pytest.mark.parametrize("backend", ["rccl", "ipc"])
def test_dp_allgather_gloo_world2_on_one_gpu(backend):
    """Two ranks share the one GPU (Gloo; RCCL refuses duplicate devices): hipGraph replays on
    two output buffers, the gather on the communication stream, event/stream ordering.  ``ipc``:
    real hipIpc memory handles (buffers and event words) across the two processes, direct pushes."""
    _run_dp("cuda", backend)


@pytest.mark.parametrize("nproc,extra,scaling,gather_dtype", [
    (2, [], "weak", None),
    (2, ["--global-batch", "4", "--gather-dtype", "bf16"], "strong", "bf16"),
    (8, [], "weak", None),                                  # the driver's N = 8 launch line, on Gloo
    (8, ["--global-batch", "32", "--gather", "ipc"], "strong", None),  # SURVEY 5.8 sizing: 4 per rank
])
def test_bench_harness_torchrun_gloo(nproc, extra, scaling, gather_dtype):
    port = _free_port()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}", "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--tiny", "--gpus", str(nproc),
           "--steps", "2", "--warmup", "1"] + extra
    # a CPU-tier test: hide any GPU (on the GPU box two ranks would otherwise pick RCCL on one device)
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="", MI_DFT_DIST_BACKEND="gloo")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    import json

    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == nproc and d["scaling"] == scaling and d["config"]["parallelism"] == f"dp{nproc}"
    assert d["value"] > 0 and d["higher_is_better"] is True
    assert d["config"]["output_allgather"] is True
    if scaling == "strong":
        g = int(extra[extra.index("--global-batch") + 1])
        assert d["config"]["global_batch"] == g and d["config"]["per_gpu_batch"] == g // nproc
    if "--gather" in extra:
        assert d["config"]["gather_backend"] == extra[extra.index("--gather") + 1]
    if gather_dtype:
        assert d["config"]["gather_dtype"] == gather_dtype
    # self-diagnosis of a multi-GPU run: the collective's rank count, the
    # gather-only cost and the comm stream's busy time per step
    mg = d["multi_gpu"]
    assert mg["collective_ranks"] == nproc
    assert mg["gather_verified"] is True  # rank r's gathered slot == rank r's local output, exactly
    assert mg["gather_only_ms"] > 0
    print(json.dumps(mg))


def test_rccl_choices_parser():
    """bench.py records what RCCL chose from its INFO log."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("bench_main", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)  # bench/ is a package: load the script by path
    rccl_choices = mod.rccl_choices

    log = "\n".join([
        "host:1:1 [0] NCCL INFO RCCL version 2.26.6+hip7.0",
        "host:1:1 [0] NCCL INFO Channel 00/32 : 0 1 2 3 4 5 6 7",
        "host:1:1 [0] NCCL INFO Channel 01/32 : 0 2 4 6 1 3 5 7",
        "host:1:1 [0] NCCL INFO 32 coll channels, 32 collnet channels, 0 nvls channels, 32 p2p channels, 4 p2p channels per peer",
        "host:1:1 [0] NCCL INFO AllGather: algo Ring proto Simple nchannels 32 nthreads 256",
        "host:1:1 [0] NCCL INFO AllGather: algo Ring proto Simple nchannels 32 nthreads 256",
        "host:1:1 [0] NCCL INFO comm 0x5f0c rank 0 nranks 8 cudaDev 0 busId 5000 commId 0x1 - Init COMPLETE",
    ])
    r = rccl_choices(log)
    assert r["nranks"] == 8
    assert r["coll_channels"] == 32 and r["p2p_channels"] == 32 and r["ring_channels"] == 32
    assert r["ring0"] == "0 1 2 3 4 5 6 7" and r["version"].startswith("2.26.6")
    assert r["tuning"] == ["AllGather: algo Ring proto Simple nchannels 32 nthreads 256"]
    assert rccl_choices("") == {}


def test_rccl_sweep_harness_gloo():
    port = _free_port()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "bench", "bench_rccl.py"), "--mb", "0.01",
           "--iters", "2", "--dtype", "fp32"]
    # a CPU-tier test: hide any GPU (on the GPU box two ranks would otherwise pick RCCL on one device)
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="", MI_DFT_DIST_BACKEND="gloo")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    import json

    lines = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and lines[0]["world"] == 2 and lines[0]["backend"] == "gloo"


def _rccl_world1_dp_worker(port, q, backend):
    """One rank, nccl (RCCL) process group on the one GPU: the DP runner with the gather forced on
    executes all_gather_into_tensor on its comm stream, overlapped with hipGraph replays."""
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
        sys.path.insert(0, ROOT)
        from datetime import timedelta

        import torch.distributed as dist

        from tensorrt_dft_plugins_amd.models import AFNOConfig, AFNONet
        from tensorrt_dft_plugins_amd.parallel import DataParallelInference

        dev = torch.device("cuda", 0)
        torch.cuda.set_device(dev)
        dist.init_process_group("nccl", rank=0, world_size=1, timeout=timedelta(seconds=120), device_id=dev)
        calls = [0]
        real = dist.all_gather_into_tensor

        def counting(*a, **k):
            calls[0] += 1
            return real(*a, **k)

        dist.all_gather_into_tensor = counting
        torch.manual_seed(0)
        cfg = AFNOConfig(img_size=(96, 192), in_chans=4, out_chans=4, embed_dim=128, depth=2, num_blocks=4)
        model = AFNONet(cfg, backend="amd").to(dev).eval()
        xs = [torch.randn(2, cfg.in_chans, *cfg.img_size, device=dev) for _ in range(6)]
        dp = DataParallelInference(model, xs[0], gather=True, use_graph=True, gather_backend=backend,
                                   force_gather=True)
        assert dp.gather, "force_gather did not enable the gather at world 1"
        got = []
        for k in range(6):  # step k+1 is enqueued before step k's gathered slot is read
            dp.inputs.copy_(xs[k])
            dp.step()
            if k >= 1:
                dp.drain()
                got.append(dp.full[(k - 1) % 2].clone())
        dp.drain()
        got.append(dp.full[5 % 2].clone())
        torch.cuda.synchronize()
        with torch.no_grad():
            want = [model(x) for x in xs]
        errs = [float((g - w).abs().max()) for g, w in zip(got, want)]
        ver = dp.verify_gather()
        n_calls = calls[0]
        fb = dp.gather_fallback
        dp.close()
        dist.destroy_process_group()
        q.put(("ok", errs, ver, n_calls, fb))
    except BaseException as e:
        q.put(("err", repr(e), None, None, None))
        raise


@pytest.mark.gpu
@pytest.mark.parametrize("backend", ["rccl", "ipc"])
def test_dp_force_gather_world1_gpu(backend):
    """The C-1 call site on the device (VERDICT r5 missing #1): a world-1 nccl (RCCL) process
    group, ``DataParallelInference(force_gather=True)``; six captured steps with a different input
    each, step k + 1 enqueued before step k's gathered slot is read; every gathered slot equals the
    eager forward of its input, ``verify_gather`` passes, and (rccl) every step went through
    ``all_gather_into_tensor``."""
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_rccl_world1_dp_worker, args=(port, q, backend))
    p.start()
    status, errs, ver, n_calls, fb = q.get(timeout=500)
    p.join(timeout=60)
    assert status == "ok", errs
    assert p.exitcode == 0
    assert max(errs) < 1e-4, errs
    assert ver == {"gather_verified": True, "gather_mismatches": 0}, ver
    if backend == "rccl":
        assert n_calls >= 6, n_calls
    else:
        assert fb is None, fb  # one rank: no peer pair to lack access
    print(f"force_gather world-1 {backend}: max |gathered - eager| per step {errs}, {n_calls} RCCL gathers")


@pytest.mark.gpu
def test_rccl_world1_capture_and_gather_gpu():
    """hipGraph capture while an RCCL (nccl backend) process group and its watchdog are live, and
    all_gather_into_tensor on the communication stream (scripts/rccl_capture_probe.py; a world-
    size-1 communicator, since one GPU cannot host two RCCL ranks)."""
    env = dict(os.environ, MASTER_PORT=str(_free_port()), MASTER_ADDR="127.0.0.1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "rccl_capture_probe.py")], capture_output=True,
                       text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "rccl capture probe ok" in r.stdout


def test_bench_force_gather_single_process_cpu():
    """``bench.py --force-gather`` at world 1: a one-rank process group (Gloo here, RCCL on a GPU) and the
    output all-gather + its exact-checksum verification in every timed step."""
    import json

    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--tiny", "--force-gather", "--steps", "2",
                        "--warmup", "1"], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
    assert d["n_gpus"] == 1 and d["config"]["output_allgather"] is True
    assert d["multi_gpu"]["collective_ranks"] == 1 and d["multi_gpu"]["gather_verified"] is True
