"""The shard transports (csrc/transport.h) on their own: dropest_test_transport drives one all-to-all(v) through exchange, the same
transfer through exchange_at with offsets that are not the prefix sums, and one gather_dev, on three small patterned arrays (elements of
8, 4 and 1 bytes) whose count matrix holds zeros, a whole zero row and column, a 1 and a block beyond 256 elements -- every received
element, every block length, every gap between the pieces and the kept block of an in-place array is checked.  The planes: local (the
threads of one process), shm (processes sharing GPU 0, as in test_gpu_multiproc.py) and RCCL (one process per GPU; needs two GPUs)."""
import ctypes as C
import multiprocessing as mp
import os

import numpy as np
import pytest

from dropest_amd import capi

pytestmark = pytest.mark.gpu
IN_PLACE = [0, 0b011]


@pytest.mark.parametrize("in_place", IN_PLACE)
@pytest.mark.parametrize("world", [1, 2, 3])
def test_local_plane(world, in_place):
    L = capi.lib()
    rc = L.dropest_test_transport(0, 0, world, None, 0, in_place)
    assert rc == 0, (rc, L.dropest_last_error().decode())


def _worker(rank, world, uid, device, dataplane, in_place, q):
    os.environ.pop("DROPEST_SHARD_DATAPLANE", None)         # (before the library loads)
    if dataplane:
        os.environ["DROPEST_SHARD_DATAPLANE"] = dataplane
    os.environ["DROPEST_MAILBOX_TIMEOUT_S"] = "20"          # a peer that died fails the collective well inside the parent's time-out
    from dropest_amd import capi as cp
    L = cp.lib()
    ub = np.frombuffer(uid, np.uint8).copy()
    rc = L.dropest_test_transport(1, rank, world, ub.ctypes.data, device, in_place)
    q.put((rank, rc, L.dropest_last_error().decode() if rc else ""))


def _run_processes(world, uid, devices, dataplane, in_place):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, uid, devices[r], dataplane, in_place, q)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(60)
    hung = [p for p in procs if p.is_alive()]
    for p in hung:
        p.kill()
    assert not hung, "ranks that did not return: %s" % [procs.index(p) for p in hung]
    got = sorted(q.get(timeout=5) for p in procs if p.exitcode == 0)
    assert [p.exitcode for p in procs] == [0] * world and [(r, rc) for r, rc, _ in got] == [(r, 0) for r in range(world)], got


@pytest.mark.parametrize("in_place", IN_PLACE)
@pytest.mark.parametrize("world", [2, 3])
def test_shm_plane_across_processes(world, in_place):
    uid = np.random.default_rng(os.getpid() + world).integers(0, 256, 128, dtype=np.uint8).tobytes()
    _run_processes(world, uid, [0] * world, "shm", in_place)


@pytest.mark.parametrize("in_place", IN_PLACE)
def test_rccl_plane_one_process_per_gpu(in_place):
    L = capi.lib()
    if L.dropest_dev_count() < 2:
        pytest.skip("the RCCL plane needs two GPUs (one rank per device)")
    uid = (C.c_uint8 * 128)()
    assert L.dropest_shard_unique_id(uid) == 0, L.dropest_last_error()
    _run_processes(2, bytes(uid), [0, 1], "", in_place)
