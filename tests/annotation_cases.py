"""Seeded annotation files and query lists for the annotation tests (annotation_model.py, test_annotation_model_cpu.py,
test_gpu_annotation.py, test_gpu_bam.py).  Every file is written into a directory of the caller (tmp_path); the records
written come back beside the path, so that the model works from what the generator wrote and not from a parser.

Streams: `sparse` (the shape test_gpu_annotation.py has drawn so far), `dense` / `dense_introns` (loci of 2-40
transcripts over the same bases, without / with explicit intron records), `far` (records just below 2^31, and a
chromosome with one one-base exon at position 0), `bed` (refFlat style: the isoforms of a gene under one label, in file
order -- not a simple file in the model's sense, see annotation_model.py)."""
import bisect
import gzip
import os
import random

from annotation_model import EXON, INTRON, Annotation, Record

K_NEXT = 4                     # a boundary's queries end at it and at the next K_NEXT boundaries
STREAMS = ("sparse", "dense", "dense_introns", "far", "bed")


class Case:
    def __init__(self, name, path, records, queries, simple):
        self.name, self.path, self.records, self.queries, self.simple = name, path, records, queries, simple
        self.model = Annotation(records)
        self.chromosomes = sorted({r.chr for r in records})


def boundaries(records):
    """per chromosome, sorted: every record's start and end (a transcript's extent begins and ends at one of them)"""
    out = {}
    for r in records:
        out.setdefault(r.chr, set()).update((r.start, r.end))
    return {c: sorted(v) for c, v in out.items()}


def boundary_queries(bounds, k_next=K_NEXT):
    """position in {b-1, b, b+1} x end_position in {b'-1, b', b'+1} for b' = b and the next k_next boundaries"""
    out = []
    for chr_, bs in bounds.items():
        for i, b in enumerate(bs):
            for p in (b - 1, b, b + 1):
                if p < 0:
                    continue
                for b2 in bs[i:i + 1 + k_next]:
                    for e in (b2 - 1, b2, b2 + 1):
                        if e >= 0:
                            out.append((chr_, p, e))
    return out


def _transcript(records, rng, chr_, gene, tid, exons, introns):
    """exons: sorted, disjoint (start, end); introns: write an intron record over (nearly) every gap between them"""
    prev = None
    for s, e in exons:
        assert s < e and (prev is None or prev <= s)
        if introns and prev is not None and prev < s and rng.random() < 0.9:
            records.append(Record(chr_, INTRON, prev, s, gene, tid))
        records.append(Record(chr_, EXON, s, e, gene, tid))
        prev = e


def _exon_grid(rng, at, n):
    """n exons from `at` on: lengths with single bases, gaps with touching exons"""
    out = []
    for _ in range(n):
        ln = rng.choice([1, 1, 3, 20, 60, 150])
        out.append((at, at + ln))
        at += ln + rng.choice([0, 1, 2, 25, 80, 200])
    return out


def _sparse(rng, introns=True):
    records = []
    for chr_ in ("chr1", "chr2", "chrX"):
        for g in range(40):
            gs = rng.randrange(0, 90_000)
            for t in range(rng.randint(1, 3)):
                pos = gs + rng.randrange(0, 300)
                exons = []
                for _ in range(rng.randint(1, 6)):
                    ln = rng.choice([1, 5, 50, 200, 800])
                    exons.append((pos, pos + ln))
                    pos += ln + rng.choice([0, 0, 1, 30, 400])
                _transcript(records, rng, chr_, "N%s_%d" % (chr_, g), "T%s_%d_%d" % (chr_, g, t), exons, introns)
    return records


def _dense(rng, introns):
    records = []
    n_tr = [0]

    def tid():
        n_tr[0] += 1
        return "TD%05d" % n_tr[0]

    def isoforms(chr_, gene, grid, k, jitter=True):
        """k isoforms of one gene over one exon grid: each leaves one exon out, some move an outer boundary by a base"""
        for i in range(k):
            exons = [x for j, x in enumerate(grid) if len(grid) < 3 or j != 1 + i % (len(grid) - 2)]
            if jitter and i % 3 == 1 and exons[0][1] - exons[0][0] > 1:
                exons[0] = (exons[0][0] + 1, exons[0][1])
            if jitter and i % 4 == 2 and exons[-1][1] - exons[-1][0] > 1:
                exons[-1] = (exons[-1][0], exons[-1][1] - 1)
            _transcript(records, rng, chr_, gene, tid(), exons, introns)

    for chr_ in ("chrD1", "chrD2"):
        at, locus = 500, 0
        for kind in ["one_gene_deep", "many_genes_deep", "exactly_16", "mixed", "neighbours"] * 3 + ["mixed"] * 8 + ["one_gene_deep_shared", "neighbours", "neighbours"]:
            locus += 1
            name = "%s_L%d" % (chr_, locus)
            if kind == "one_gene_deep":                      # 17+ transcripts of ONE gene: the result set has one or two entries
                grid = _exon_grid(rng, at, rng.randint(5, 8))
                isoforms(chr_, "G" + name, grid, rng.randint(17, 40))
                end = grid[-1][1]
            elif kind == "one_gene_deep_shared":             # ... and a second gene nested in it
                grid = _exon_grid(rng, at, 8)
                isoforms(chr_, "G" + name, grid, 24)
                isoforms(chr_, "H" + name, grid[2:6], 3)
                end = grid[-1][1]
            elif kind == "many_genes_deep":                  # one transcript each of 17+ genes: more than 16 results
                k = rng.randint(18, 30)
                end = at
                for j in range(k):
                    grid = _exon_grid(rng, at + 7 * j, rng.randint(3, 5))
                    grid[-1] = (grid[-1][0], max(grid[-1][1], at + 7 * k + 40 + j))      # all of them over the locus' middle
                    _transcript(records, rng, chr_, "G%s_%02d" % (name, j), tid(), grid, introns)
                    end = max(end, grid[-1][1])
            elif kind == "exactly_16":                       # 16 transcripts of 4 genes over the same bases
                grid = _exon_grid(rng, at, 6)
                for j in range(4):
                    shifted = [(s + 2 * j, e + 2 * j) for s, e in grid] if j % 2 else grid
                    isoforms(chr_, "G%s_%d" % (name, j), shifted, 4, jitter=False)
                end = grid[-1][1] + 8
            elif kind == "mixed":                            # 2-16 transcripts of 2-5 genes: nested, overlapping, sharing exons
                grid = _exon_grid(rng, at, rng.randint(4, 9))
                n_genes, left = rng.randint(2, 5), rng.randint(2, 16)
                end = grid[-1][1]
                for j in range(n_genes):
                    k = max(1, left // (n_genes - j)) if j < n_genes - 1 else max(1, left)
                    left -= k
                    how = rng.choice(["shared", "nested", "shifted", "alternating"])
                    if how == "shared":
                        mine = grid
                    elif how == "nested":
                        mine = grid[1:-1] or grid
                    elif how == "alternating":               # exons in the others' introns
                        mine = [(e, e + max(1, (s2 - e) // 2)) for (s, e), (s2, e2) in zip(grid, grid[1:]) if s2 - e >= 2] or grid
                    else:
                        d = rng.choice([1, 2, 30])
                        mine = [(s + d, e + d) for s, e in grid]
                    isoforms(chr_, "G%s_%d" % (name, j), mine, k)
                    end = max(end, mine[-1][1] + 1)
            else:                                            # two one-transcript genes a few bases apart
                a = _exon_grid(rng, at, 2)
                b = _exon_grid(rng, a[-1][1] + rng.choice([0, 1, 12]), 2)
                _transcript(records, rng, chr_, "G%s_a" % name, tid(), a, introns)
                _transcript(records, rng, chr_, "G%s_b" % name, tid(), b, introns)
                end = b[-1][1]
            at = end + rng.choice([1, 40, 300, 1500])
    return records


FAR_TOP = 2 ** 31 - 1          # the largest end a GTF's int32-minded writers give; BAM positions are int32


def _far(rng):
    records = []
    at = FAR_TOP - 6000
    for g in range(5):
        grid = _exon_grid(rng, at, 5)
        for t in range(rng.randint(1, 4)):
            _transcript(records, rng, "chrFar", "GF%d" % g, "TF%d_%d" % (g, t), grid[t % 2:], False)
        at = grid[-1][1] - rng.choice([0, 50, -30])
        if at > FAR_TOP - 2500:
            break
    for t in range(3):                                        # up to the last base below 2^31
        _transcript(records, rng, "chrFar", "GFtop", "TFtop_%d" % t, [(FAR_TOP - 400 - t, FAR_TOP - 300), (FAR_TOP - 100, FAR_TOP - 50 - t), (FAR_TOP - 1 - t, FAR_TOP)], False)
    assert all(r.end <= FAR_TOP for r in records)
    records.append(Record("chrZero", EXON, 0, 1, "GZero", "TZero"))
    return records


def _bed(rng):
    """refFlat style: every line carries the gene's label only, the isoforms of a gene follow each other in file order"""
    records = []
    for chr_ in ("chrB1", "chrB2"):
        at = 200
        for g in range(60):
            label = "B%s_%d" % (chr_, g)
            grid = _exon_grid(rng, at, rng.randint(3, 8))
            for iso in range(rng.randint(1, 6)):
                how = rng.choice(["same", "skip", "nested", "shifted", "longer"])
                if how == "same":
                    mine = list(grid)
                elif how == "skip":
                    mine = [x for j, x in enumerate(grid) if j != 1 + iso % max(1, len(grid) - 2)]
                elif how == "nested":
                    mine = [(s + 1, max(s + 2, e - 1)) for s, e in grid[1:-1]] or list(grid)
                elif how == "shifted":
                    d = rng.choice([1, 5, 40])
                    mine = [(s + d, e + d) for s, e in grid]
                else:
                    mine = [(s, e + rng.choice([0, 1, 10, 100])) for s, e in grid]
                for s, e in mine:                                                  # (an isoform's own exons may overlap here: BED says nothing against it)
                    records.append(Record(chr_, EXON, s, e, label, label))
            at = grid[-1][1] + rng.choice([-200, -20, 0, 1, 50, 900])               # genes overlap their neighbours
            at = max(at, 0)
    return records


def _write(path, records, bed):
    lines = []
    for n, r in enumerate(records):
        if bed:
            lines.append("%s\t%d\t%d\t%s" % (r.chr, r.start, r.end, r.gene))
        else:
            # the name of a gene is its gene_name where there is one, else its gene_id (GtfRecord::gene_name): both spellings
            ids = 'gene_id "%s";' % r.gene if _id_only(r.gene) else 'gene_id "id_%s"; gene_name "%s";' % (r.gene, r.gene)
            lines.append('%s\tsrc\t%s\t%d\t%d\t.\t+\t.\t%s transcript_id "%s"; tss_id "x";' % (r.chr, "exon" if r.type == EXON else "intron", r.start + 1, r.end, ids, r.transcript))
    with gzip.open(path, "wt") as f:
        f.write("\n".join(lines) + "\n")


def _id_only(name):
    """a choice per gene that does not depend on the interpreter's string hashing"""
    return sum(name.encode()) % 3 == 0


def make(tmp_path, stream, seed=1, n_background=3000, n_cross=6000):
    """-> Case: the file written under tmp_path, its records, its queries (chromosome, position, end_position)"""
    rng = random.Random("%s/%d" % (stream, seed))
    bed = stream == "bed"
    records = {"sparse": lambda: _sparse(rng), "dense": lambda: _dense(rng, False), "dense_introns": lambda: _dense(rng, True),
               "far": lambda: _far(rng), "bed": lambda: _bed(rng)}[stream]()
    path = os.path.join(str(tmp_path), "%s_%d.%s.gz" % (stream, seed, "bed" if bed else "gtf"))
    _write(path, records, bed)
    bounds = boundaries(records)
    queries = boundary_queries(bounds)
    for chr_, bs in bounds.items():
        near = sorted({b + d for b in bs for d in (-1, 0, 1) if b + d >= 0})
        lo, hi = bs[0], bs[-1]
        # pairs of boundary points further apart than the next few boundaries (reads that begin in one locus and end in another)
        for _ in range(n_cross // len(bounds)):
            p = rng.choice(near)
            q = rng.choice(near)
            if abs(p - q) > 4000:
                q = near[min(len(near) - 1, bisect.bisect_left(near, p + rng.randrange(1, 2500)))]
            p, q = min(p, q), max(p, q)
            queries.append((chr_, p, q + rng.choice([0, 1])))
        # end_position == 0, == position; positions past the last piece; a uniform background
        queries += [(chr_, p, 0) for p in (0, 1, lo, max(0, lo - 1), hi - 1, hi)]
        queries += [(chr_, p, p) for p in rng.sample(near, min(50, len(near)))]
        queries += [(chr_, hi + d, hi + d + e) for d in (0, 1, 2, 1000) for e in (0, 1, 50)] + [(chr_, hi - 1, hi + 1000), (chr_, max(0, hi - 5000), hi + 1)]
        for _ in range(n_background // len(bounds)):
            p = rng.randrange(max(0, lo - 2000), hi + 2000)
            queries.append((chr_, p, p + rng.randrange(1, 400)))
    some = bounds[sorted(bounds)[0]]
    queries += [("chrNope", b, b + 40) for b in some[:20]] + [("chrNope", 0, 0)]
    assert all(0 <= p < 2 ** 32 - 1 and 0 <= e < 2 ** 32 for _, p, e in queries)
    return Case(stream, path, records, queries, simple=not bed)
