"""Developer tool: what dropest_read_corrections (`dropest -F`, csrc/k_readfix.h + csrc/read_corrections.h) costs on a synthetic C2-like
container (10x-shaped stream over a whitelist, 5 000 real cells, whitelist barcode merge), with HIP events around its launches.
    python scripts/bench_read_corrections.py [reads, default 2e7]
Two containers over the same reads: the default UMI merge without the merge targets (the source map is empty), and -u with the targets
kept (on this stream about a thousand sources: the synthetic UMIs are rarely one base apart).  Each runs its pass twice (the second reuses the context's buffers) and prints, per run: the reads per verdict,
the wall time of the call, the kernel's time and algorithmic bytes, the sorts that build the two key arrays, and the sources kept.
No threshold: nobody has measured this before."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dropest_amd import capi
from dropest_amd.synth import SynthStream

n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 20_000_000
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
