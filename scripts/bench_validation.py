"""Developer tool: wall time of the merge validation statistics (`dropest -S`) at the reference's sample sizes -- 1 000 000 distant pairs
(banded distance 5 .. 100) and 100 000 adjacent pairs (exactly 1) -- on a synthetic C2-like container (10x-shaped stream over a whitelist,
5 000 real cells; the reads go through the whitelist merge first, as `dropest -m -S` would have it).
    python scripts/bench_validation.py [reads, default 2e7] [max_draws, default 2^30]
Prints, per sample: pairs found, candidates drawn, sampler rounds, evaluation chunks, and ms for the view (built once for both samples),
the sampler and the evaluation.  No threshold: nobody has measured this before."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dropest_amd import capi
from dropest_amd.synth import SynthStream

n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 20_000_000
max_draws = int(float(sys.argv[2])) if len(sys.argv) > 2 else 1 << 30
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
