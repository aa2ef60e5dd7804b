"""Developer tool: wall time of the merge validation statistics (`dropest -S`) at the reference's sample sizes -- 1 000 000 distant pairs
(banded distance 5 .. 100) and 100 000 adjacent pairs (exactly 1) -- on a synthetic C2-like container (10x-shaped stream over a whitelist,
5 000 real cells; the reads go through the whitelist merge first, as `dropest -m -S` would have it).
    python scripts/bench_validation.py [reads, default 2e7] [max_draws, default 2^30] [--shards N]
Prints, per sample: pairs found, candidates drawn, sampler rounds, evaluation chunks, and ms for the view (built once for both samples),
the sampler and the evaluation.  No threshold: nobody has measured this before.
--shards N: the same stream then runs through ShardGroup([0] * N) -- N shards on device 0, so they share what the one context had to
itself and cannot beat it; the gather of the view crosses no link -- and the phases of the sharded statistics are printed per shard (keys
of the own cells / gather + place / rows and tables / sampler / evaluation, ms over both runs' second) next to the one context's."""
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
max_draws = int(float(argv[1])) if len(argv) > 1 else 1 << 30
s = SynthStream(n_reads=n, n_cells=5000, n_genes=30000, cb_len=16, umi_len=10)
cb, umi, gene, aux = s.generate_host()
c = capi.Context(merge_kind=capi.MERGE_REAL_BARCODES, barcodes_kind=capi.BARCODES_CONST, barcodes_file=s.whitelist_path,
                 min_genes_before_merge=20, min_genes_after_merge=100)
c.push_reads(cb, umi, gene, aux)
c.set_initialized()
c.merge_and_filter()
print("reads %d, cells %d, filtered cells %d, molecules %d" % (n, c.total_cells_number(), len(c.filtered_cells()), c.table_sizes()["molecules"]))
for attempt in range(2):                                            # the second run reuses the context's buffers
    t0 = time.time()
    distant, adjacent = c.merge_validation((5, 100, 1_000_000), (1, 1, 100_000), max_draws=max_draws)
    wall = (time.time() - t0) * 1e3
    print("run %d: wall %.1f ms, view %.1f ms" % (attempt, wall, distant["ms_view"]))
    for name, r in (("distant", distant), ("adjacent", adjacent)):
        print("  %-8s found %d (complete %d), draws %d, rounds %d, chunks %d, sampler %.1f ms, evaluation %.1f ms"
              % (name, r["n_found"], r["complete"], r["draws_used"], r["rounds"], r["chunks"], r["ms_sampler"], r["ms_evaluation"]))
c.close()

if shards > 0:
    from dropest_amd.multi import ShardGroup
    g = ShardGroup([0] * shards, merge_kind=capi.MERGE_REAL_BARCODES, barcodes_kind=capi.BARCODES_CONST, barcodes_file=s.whitelist_path,
                   min_genes_before_merge=20, min_genes_after_merge=100)
    for i, sh in enumerate(g.shards):
        lo, hi = n * i // shards, n * (i + 1) // shards
        sh.set_reads(capi.DeviceArrays.from_host(0, cb[lo:hi], umi[lo:hi], gene[lo:hi], aux[lo:hi]), lo)
    g.step()
    print("%d shards on device 0, filtered cells %d" % (shards, len(g.shards[0].matrix(True)[3])))
    names = ("validation:keys", "validation:gather_place", "validation:rows_tables", "validation:sampler", "validation:evaluation")
    for attempt in range(2):
        for sh in g.shards:
            sh.set_option("reset_phase_stats", 1)
        t0 = time.time()
        distant, adjacent = g.merge_validation((5, 100, 1_000_000), (1, 1, 100_000), max_draws=max_draws)
        wall = (time.time() - t0) * 1e3
        print("sharded run %d: wall %.1f ms, view %.1f ms (shard 0)" % (attempt, wall, distant["ms_view"]))
        for name, r in (("distant", distant), ("adjacent", adjacent)):
            print("  %-8s found %d (complete %d), draws %d, rounds %d, chunks %d, sampler %.1f ms, evaluation %.1f ms (shard 0)"
                  % (name, r["n_found"], r["complete"], r["draws_used"], r["rounds"], r["chunks"], r["ms_sampler"], r["ms_evaluation"]))
        for i, sh in enumerate(g.shards):
            ph = sh.phase_stats()
            print("  shard %d: " % i + ", ".join("%s %.1f ms" % (k.split(":")[1], ph.get(k, {"ms": 0.0})["ms"]) for k in names)
                  + ", gathered %.1f MB" % (ph.get("validation:gather_place", {"bytes": 0.0})["bytes"] / 1e6))
    g.close()
