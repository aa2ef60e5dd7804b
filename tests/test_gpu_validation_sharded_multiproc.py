"""`dropest -S` with one PROCESS per shard (dropest_shard_merge_validation_samples over the multi-process transport): two processes
share device 0, so the view's blocks cross through POSIX shared memory (DROPEST_SHARD_DATAPLANE=shm) and the host collectives through the
mailbox, as in test_gpu_multiproc.py.  The case is `whitelist` (a barcode merge across the shards in front of the statistics); rank 0's
samples are bit-equal to those of the same two shards inside one process."""
import ctypes as C
import multiprocessing as mp
import os
import tempfile

import numpy as np
import pytest

from dropest_amd import capi
from dropest_amd.multi import ShardGroup

import validation_cases as vc

pytestmark = pytest.mark.gpu

KEYS = ("cell1", "cell2", "umis1", "umis2", "edit_distance", "intersection", "expected", "probability")
SCALARS = ("n_found", "draws_used", "complete", "rounds", "chunks")


def _worker(rank, world, uid, cfg_kw, side, npz, out, samples, cap):
    try:
        os.environ["DROPEST_SHARD_DATAPLANE"] = "shm"
        from dropest_amd import capi as cp
        from dropest_amd.multi import Shard
        L = cp.lib()
        cfg, keep = cp.make_cfg(device=0, **cfg_kw)
        h = C.c_void_p()
        ub = np.frombuffer(uid, np.uint8).copy()
        rc = L.dropest_shard_create(C.byref(cfg), rank, world, ub.ctypes.data, C.byref(h))
        assert rc == 0, L.dropest_last_error()
        sh = Shard(h.value)
        d = np.load(npz)
        n = len(d["cb"])
        lo, hi = n * rank // world, n * (rank + 1) // world
        if side:
            sh.set_side_strings(side)
        sh.set_reads(cp.DeviceArrays.from_host(0, d["cb"][lo:hi], d["umi"][lo:hi], d["gene"][lo:hi], d["aux"][lo:hi]), lo)
        sh.step()
        got = sh.merge_validation(*samples, max_draws=cap)
        if rank == 0:
            flat = {"col": sh.matrix(True)[3]}
            for i, s in enumerate(got):
                for k in KEYS:
                    flat["%s_%d" % (k, i)] = s[k]
                flat["scalars_%d" % i] = np.array([s[k] for k in SCALARS], np.int64)
            np.savez(out, **flat)
        sh.close()
    except BaseException:   # noqa: BLE001 (the parent reads the text)
        import traceback
        open(out + ".err%d" % rank, "w").write(traceback.format_exc())
        raise


def test_two_processes_equal_the_in_process_group(tmp_path):
    c = vc.case("whitelist")
    cb, umi, gene, aux, side = c.arrays()
    kw = dict(c.ctx, barcodes_file=c.whitelist(tmp_path))
    samples = [(lo, hi, n) for lo, hi, n, _, _ in c.samples]
    cap = max(s[3] for s in c.samples)
    world = 2
    tmp = tempfile.mkdtemp(prefix="dropest_val_mp_")
    npz, out = os.path.join(tmp, "reads.npz"), os.path.join(tmp, "out.npz")
    np.savez(npz, cb=cb, umi=umi, gene=gene, aux=aux)
    uid = np.random.default_rng(os.getpid()).integers(0, 256, 128, dtype=np.uint8).tobytes()
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_worker, args=(r, world, uid, kw, tuple(side), npz, out, samples, cap)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(600)
    errs = [open(out + ".err%d" % r).read() for r in range(world) if os.path.exists(out + ".err%d" % r)]
    assert not errs and all(p.exitcode == 0 for p in procs), "\n".join(errs) or [p.exitcode for p in procs]
    got = np.load(out)

    g = ShardGroup([0] * world, **kw)
    try:
        n = len(cb)
        for i, s in enumerate(g.shards):
            if side:
                s.set_side_strings(side)
            lo, hi = n * i // world, n * (i + 1) // world
            s.set_reads(capi.DeviceArrays.from_host(0, cb[lo:hi], umi[lo:hi], gene[lo:hi], aux[lo:hi]), lo)
        g.step()
        want = g.merge_validation(*samples, max_draws=cap)
        assert np.array_equal(got["col"], g.shards[0].matrix(True)[3])
    finally:
        g.close()
    assert len(want) == len(samples) and sum(w["n_found"] for w in want) > 0
    for i, w in enumerate(want):
        for k in KEYS:
            x, y = np.ascontiguousarray(got["%s_%d" % (k, i)]), np.ascontiguousarray(w[k])
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (i, k)
        assert [int(v) for v in got["scalars_%d" % i]] == [int(w[k]) for k in SCALARS], i
