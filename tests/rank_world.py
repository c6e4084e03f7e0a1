"""The launcher of the ranks tests: `world` processes of one program that share the one GPU, every one under a time limit of
its own, the first to exit non-zero ending the others -- nothing goes on using the GPU behind a failure."""
import os
import socket
import subprocess
from concurrent.futures import ThreadPoolExecutor, as_completed

LIMIT = 120          # seconds a rank may take (a healthy run takes a few)


def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def run_world(argv, world, env=None):
    """start `argv` once per rank r = 0 .. world - 1 with RANK, WORLD_SIZE, LOCAL_RANK = r, MASTER_ADDR, a free MASTER_PORT,
    OMP_NUM_THREADS = 1 and HSA_ENABLE_IPC_MODE_LEGACY = 0 over the caller's environment, and the dict `env` over those.
    Returns (procs, outs): the finished processes and their stdout + stderr, by rank.  Fails with the output of the first rank that exited non-zero, if one did."""
    port = free_port()
    procs = []
    for r in range(world):
        renv = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1",
                    MASTER_PORT=str(port), OMP_NUM_THREADS="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
        renv.update(env or {})
        procs.append(subprocess.Popen(["timeout", "-k", "10", str(LIMIT), *argv], env=renv, stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT, text=True))
    outs, failed = [None] * world, None
    with ThreadPoolExecutor(max_workers=world) as pool:
        waits = {pool.submit(p.communicate): r for r, p in enumerate(procs)}
        for done in as_completed(waits):
            r = waits[done]
            outs[r] = done.result()[0]
            if procs[r].returncode != 0 and failed is None:
                failed = r
                for q in procs:
                    if q.poll() is None:
                        q.terminate()
    assert failed is None, f"rank {failed} of {world} failed first (exit {procs[failed].returncode}):\n{outs[failed][-3000:]}"
    return procs, outs
