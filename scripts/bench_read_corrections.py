"""Developer tool: what dropest_read_corrections (`dropest -F`, csrc/k_readfix.h + csrc/read_corrections.h) costs on a synthetic C2-like
container (10x-shaped stream over a whitelist, 5 000 real cells, whitelist barcode merge), with HIP events around its launches.
    python scripts/bench_read_corrections.py [reads, default 2e7] [--shards N]
Two containers over the same reads: the default UMI merge without the merge targets (the source map is empty), and -u with the targets
kept (on this stream about a thousand sources: the synthetic UMIs are rarely one base apart).  Each runs its pass twice (the second reuses the context's buffers) and prints, per run: the reads per verdict,
the wall time of the call, the kernel's time and algorithmic bytes, the sorts that build the two key arrays, and the sources kept.
No threshold: nobody has measured this before.
--shards N: the same two configurations then run through ShardGroup([0] * N) -- N shards on device 0, so they share the CUs the one context had
to itself: the run shows the work a sharded container adds (the column table, the gathered view), not a speed-up, and its gathers cross no
link.  Per shard and run: the phases of dropest_shard_read_corrections in host ms (table = lists + gather + insert; keys / gather_place = the
molecule view; the sources; the kernel's phase; the whole call) and the decision kernel under HIP events."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dropest_amd import capi
from dropest_amd.synth import SynthStream

argv = sys.argv[1:]
shards = 0
if "--shards" in argv:
    at = argv.index("--shards")
    shards = int(argv[at + 1])
    del argv[at:at + 2]
n = int(float(argv[0])) if len(argv) > 0 else 20_000_000
s = SynthStream(n_reads=n, n_cells=5000, n_genes=30000, cb_len=16, umi_len=10)
cb, umi, gene, aux = s.generate_host()
for name, kw, save in (("simple UMI merge, targets not kept", {}, False),
                       ("-u, targets kept", dict(umi_merge_kind=capi.UMI_MERGE_DIRECTIONAL), True)):
    c = capi.Context(merge_kind=capi.MERGE_REAL_BARCODES, barcodes_kind=capi.BARCODES_CONST, barcodes_file=s.whitelist_path,
                     min_genes_before_merge=20, min_genes_after_merge=100, **kw)
    c.set_save_umi_merge_targets(save)
    c.push_reads(cb, umi, gene, aux)
    print("%s: %d reads" % (name, n))
    for attempt in range(2):
        c.set_profiling(False)
        c.set_initialized()
        c.merge_and_filter()
        c.set_profiling(True, only="read_corrections")
        before = c.kernel_stats()
        t0 = time.time()
        counts = c.read_correction_counts()
        wall = (time.time() - t0) * 1e3
        after = c.kernel_stats()
        print("  run %d: cells %d, filtered %d, molecules %d, sources %d; verdicts %s; wall %.2f ms"
              % (attempt, c.total_cells_number(), len(c.filtered_cells()), c.table_sizes()["molecules"], len(c.umi_merge_targets()[0]),
                 counts.tolist(), wall))
        for k in sorted(after):
            d = {f: after[k][f] - before.get(k, dict(launches=0, ms=0.0, bytes=0.0))[f] for f in ("launches", "ms", "bytes")}
            if d["launches"]:
                print("    %-36s %3d launches %8.3f ms %10.1f MB" % (k, d["launches"], d["ms"], d["bytes"] / 1e6))
        c.reset_results()
    c.close()
    if shards > 0:
        from dropest_amd.multi import ShardGroup
        g = ShardGroup([0] * shards, merge_kind=capi.MERGE_REAL_BARCODES, barcodes_kind=capi.BARCODES_CONST, barcodes_file=s.whitelist_path,
                       min_genes_before_merge=20, min_genes_after_merge=100, **kw)
        for i, sh in enumerate(g.shards):
            lo, hi = n * i // shards, n * (i + 1) // shards
            sh.ctx.set_save_umi_merge_targets(save)
            sh.set_reads(capi.DeviceArrays.from_host(0, cb[lo:hi], umi[lo:hi], gene[lo:hi], aux[lo:hi]), lo)
        names = ("read_corrections:table", "read_corrections:keys", "read_corrections:gather_place", "read_corrections:source_keys",
                 "read_corrections:source_gather_place", "read_corrections:kernel", "read_corrections")
        for attempt in range(2):
            for sh in g.shards:
                sh.ctx.set_profiling(False)
            g.step()
            for sh in g.shards:
                sh.set_option("reset_phase_stats", 1)
                sh.ctx.set_profiling(True, only="read_corrections")
            before = [sh.ctx.kernel_stats() for sh in g.shards]
            t0 = time.time()
            counts = g.read_correction_counts()
            wall = (time.time() - t0) * 1e3
            print("  %d shards, run %d: filtered %d; verdicts %s; wall %.2f ms" % (shards, attempt, len(g.shards[0].matrix(True)[3]), counts.tolist(), wall))
            for i, sh in enumerate(g.shards):
                ph, after = sh.phase_stats(), sh.ctx.kernel_stats()
                k = after.get("read_corrections_shard", dict(launches=0, ms=0.0))
                k0 = before[i].get("read_corrections_shard", dict(launches=0, ms=0.0))
                print("    shard %d: " % i + ", ".join("%s %.2f" % (x.split(":")[-1] if ":" in x else "call", ph.get(x, {"ms": 0.0})["ms"]) for x in names)
                      + " ms; kernel (events) %.3f ms; table gathered %.3f MB, view gathered %.1f MB"
                      % (k["ms"] - k0["ms"], ph.get("read_corrections:table", {"bytes": 0.0})["bytes"] / 1e6,
                         ph.get("read_corrections:gather_place", {"bytes": 0.0})["bytes"] / 1e6))
        g.close()
