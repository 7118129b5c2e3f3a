"""Multi-process test plumbing with a bound on every wait: gloo groups whose collectives time out, and a spawn whose join has a
deadline.  A rank that dies inside a collective otherwise leaves its peers waiting for gloo's default 30 minutes -- on the GPU
tests, holding the device all that time."""
import os
import socket
import time
from datetime import timedelta


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def init_gloo(rank, world, port, seconds):
    """Join the gloo group of `world` local ranks; every collective of the group raises after `seconds` instead of waiting."""
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=timedelta(seconds=seconds))


def spawn_and_join(fn, args, nprocs, deadline_s, poll_s=2.0):
    """torch.multiprocessing.spawn(fn, args, nprocs) joined within `deadline_s` seconds.  A worker that raises surfaces as
    ProcessRaisedException with its traceback (mp.spawn's own behaviour; its peers are terminated by the context).  When the
    deadline passes every child is terminated, those still alive after 10 s are killed, and TimeoutError is raised.  Nothing is
    ever spawned a second time."""
    import torch.multiprocessing as mp

    ctx = mp.spawn(fn, args=args, nprocs=nprocs, join=False)
    end = time.monotonic() + deadline_s
    try:
        while True:
            left = end - time.monotonic()
            if left <= 0:
                break
            if ctx.join(timeout=min(poll_s, left)):
                return
    except BaseException:
        _stop(ctx.processes)
        raise
    _stop(ctx.processes)
    raise TimeoutError(f"spawn_and_join: {nprocs} worker(s) of {getattr(fn, '__name__', fn)} still running after {deadline_s:g} s; terminated")


def _stop(processes, grace_s=10.0):
    for p in processes:
        if p.is_alive():
            p.terminate()
    end = time.monotonic() + grace_s
    for p in processes:
        p.join(max(0.0, end - time.monotonic()))
    for p in processes:
        if p.is_alive():
            p.kill()
    for p in processes:
        p.join(5.0)
