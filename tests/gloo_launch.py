"""The two ends of a multi-process test: run_ranks starts the ranks of a worker script from a test, and a worker script's
main runs inside gloo_group."""
import contextlib
import os
import socket
import subprocess
import sys

TESTS = os.path.dirname(os.path.abspath(__file__))


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def run_ranks(worker_script, world, args, timeout, local_rank=None):
    """Starts `world` ranks of tests/<worker_script> with the command-line `args`; every rank must exit 0, each within `timeout`
    seconds of the wait for it.  No rank outlives the call: when one fails or times out, the others -- blocked in a collective
    that will never complete -- are killed and reaped before the assertion propagates.  local_rank: LOCAL_RANK of every rank
    (the GPU tests put all ranks on device "0"); None leaves it unset."""
    env = dict(os.environ, WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(free_port()))
    if local_rank is not None:
        env["LOCAL_RANK"] = str(local_rank)
    cmd = [sys.executable, os.path.join(TESTS, worker_script)] + [str(a) for a in args]
    procs = []
    try:
        for r in range(world):
            procs.append(subprocess.Popen(cmd, env=dict(env, RANK=str(r))))
        for r, p in enumerate(procs):
            assert p.wait(timeout=timeout) == 0, "rank %d of %s failed" % (r, worker_script)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait(timeout=30)


@contextlib.contextmanager
def gloo_group(single=True):
    """A worker's process group: yields (rank, world, dist) from RANK / WORLD_SIZE with the gloo group up; after the body a
    barrier (rank 0 has written its results by then), and the group is destroyed however the body ends.  single=False: one
    process makes no group and gets dist None, as a caller without torch.distributed would run."""
    import torch.distributed as dist
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    if world == 1 and not single:
        yield rank, world, None
        return
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        yield rank, world, dist
        dist.barrier()
    finally:
        dist.destroy_process_group()
