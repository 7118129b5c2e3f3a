"""CPU: gigapose_testing/spawn.py -- the bounded spawn every multi-process test goes through.  A worker that outlives the deadline is
terminated and the call raises; a worker that raises surfaces its traceback; a clean run returns; a gloo group made by init_gloo
gives up on a collective whose peer never arrives instead of waiting for gloo's default 30 minutes."""
import os
import time

import pytest

from gigapose_testing import spawn


def _sleeper(rank, tmp):
    with open(os.path.join(tmp, f"pid{rank}"), "w") as f:
        f.write(str(os.getpid()))
    time.sleep(120)
    with open(os.path.join(tmp, f"survived{rank}"), "w") as f:   # never reached: the parent terminates this process
        f.write("x")


def _raiser(rank, tmp):
    if rank == 1:
        raise ValueError("planted failure of rank 1")
    time.sleep(120)   # the peer is still busy when rank 1 dies: it must not keep the call waiting


def _clean(rank, tmp, port):
    import torch
    import torch.distributed as dist

    spawn.init_gloo(rank, 2, port, 60)
    try:
        t = torch.tensor([float(rank + 1)])
        dist.all_reduce(t)
        assert float(t) == 3.0
        with open(os.path.join(tmp, f"ok{rank}"), "w") as f:
            f.write("x")
    finally:
        dist.destroy_process_group()


def _lonely(rank, tmp, port):
    import torch
    import torch.distributed as dist

    spawn.init_gloo(rank, 2, port, 5)
    if rank == 1:
        time.sleep(60)      # never joins the collective
        return
    t0 = time.monotonic()
    try:
        dist.all_reduce(torch.tensor([1.0]))
    except Exception as e:   # noqa: BLE001 -- gloo raises RuntimeError / DistBackendError depending on the version
        with open(os.path.join(tmp, "gave_up"), "w") as f:
            f.write(f"{time.monotonic() - t0:.1f} {type(e).__name__}")
        raise


def _alive(pid):
    try:
        os.kill(pid, 0)
    except ProcessLookupError:
        return False
    return True


def test_a_worker_past_the_deadline_is_terminated_and_the_call_raises(tmp_path):
    t0 = time.monotonic()
    with pytest.raises(TimeoutError, match="still running after 5 s"):
        spawn.spawn_and_join(_sleeper, (str(tmp_path),), nprocs=2, deadline_s=5)
    assert time.monotonic() - t0 < 40
    pids = [int((tmp_path / f"pid{r}").read_text()) for r in range(2)]   # both had started ...
    assert not any(_alive(p) for p in pids)                               # ... and neither is left
    assert not list(tmp_path.glob("survived*"))


def test_a_worker_that_raises_surfaces_its_traceback(tmp_path):
    from torch.multiprocessing import ProcessRaisedException

    t0 = time.monotonic()
    with pytest.raises(ProcessRaisedException) as e:
        spawn.spawn_and_join(_raiser, (str(tmp_path),), nprocs=2, deadline_s=60)
    assert "planted failure of rank 1" in str(e.value) and "_raiser" in str(e.value)   # message + the frame that raised
    assert time.monotonic() - t0 < 40, "the sleeping peer held the call"


def test_a_clean_run_returns(tmp_path):
    assert spawn.spawn_and_join(_clean, (str(tmp_path), spawn.free_port()), nprocs=2, deadline_s=120) is None
    assert sorted(p.name for p in tmp_path.glob("ok*")) == ["ok0", "ok1"]


def test_a_collective_without_its_peer_gives_up_within_the_group_timeout(tmp_path):
    from torch.multiprocessing import ProcessRaisedException

    with pytest.raises(ProcessRaisedException):
        spawn.spawn_and_join(_lonely, (str(tmp_path), spawn.free_port()), nprocs=2, deadline_s=50)
    seconds = float((tmp_path / "gave_up").read_text().split()[0])
    assert seconds < 30, f"the 5 s group timeout took {seconds} s"
