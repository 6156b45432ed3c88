"""Spawned ranks for the synchronised-BatchNorm tests: every wait is bounded, a rank that raises says so at once, and nothing is left alive.

``run_ranks(target, world, args)`` starts ``world`` processes ``target(rank, world, port, q, *args)``; a target wraps its body in
``report(q, rank, body)``, which puts ``(rank, "ok", body())`` or ``(rank, "error", traceback)`` on the queue.  The parent polls the queue:
the first error, or a rank that exited without reporting, fails the call within a second instead of after the whole timeout; ranks still
alive then (blocked in a collective their peer never joined) are killed."""
import queue
import time
import traceback

import torch.multiprocessing as mp


def report(q, rank, body):
    try:
        q.put((rank, "ok", body()))
    except BaseException:
        q.put((rank, "error", traceback.format_exc()))
        raise


def run_ranks(target, world, port, args=(), timeout=400.0):
    """{rank: payload}; raises AssertionError naming the rank and its traceback otherwise."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=target, args=(r, world, port, q) + tuple(args)) for r in range(world)]
    for pr in procs:
        pr.start()
    got, problem, deadline = {}, None, time.monotonic() + timeout
    try:
        while len(got) < world and problem is None:
            try:
                rank, status, payload = q.get(timeout=1.0)
            except queue.Empty:
                dead = [r for r, pr in enumerate(procs) if r not in got and pr.exitcode is not None]
                if dead and q.empty():
                    problem = f"rank {dead[0]} exited with code {procs[dead[0]].exitcode} without reporting"
                elif time.monotonic() > deadline:
                    problem = f"no report from ranks {sorted(set(range(world)) - set(got))} within {timeout:.0f} s"
                continue
            if status == "ok":
                got[rank] = payload
            else:
                problem = f"rank {rank} raised:\n{payload}"
        if problem is None:
            for pr in procs:
                pr.join(60)
    finally:
        for pr in procs:
            if pr.is_alive():
                pr.kill()
                pr.join(30)
    assert problem is None, problem
    assert all(pr.exitcode == 0 for pr in procs), [pr.exitcode for pr in procs]
    return got
