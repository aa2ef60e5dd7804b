"""A plain model of the reference's gene annotation of a read (-g), written from the reference's text and independent of
dropest_amd/csrc/host/gene_annotation.cpp, of the kernel (csrc/annotation_api.hip) and of the oracle.

* `decide(set1, set2)`: ReadParamsParser::get_gene_from_reference and find_exon
  (Estimation/BamProcessing/ReadParamsParser.cpp:92-172) over the two result sets of a read's end points.
* `Annotation(records)`: RefGenesContainer::get_gene_info (Tools/GeneAnnotation/RefGenesContainer.cpp:182-213) by brute
  force over the records of a file: no binary search, no pieces, no flat tables.  Claimed for SIMPLE files only: every
  transcript id distinct and on one chromosome, the records of a transcript sorted and disjoint -- there the
  reference's IntervalsContainer (IntervalsContainer.h:151-238) is a plain union of its intervals.  `depth` needs no
  such condition: a transcript's extent is the hull of its records in every file (Interval::merge,
  RefGenesContainer.cpp:100-102) and enters the chromosome's container once (:88-91).
* `classify(set1, set2)`: the branch of get_gene_from_reference a read takes.

All positions 0-based, half-open, as GtfRecord keeps them (RefGenesContainer.cpp:176-177, :226-227)."""
import gzip

INTRON, EXON = "INTRON", "EXON"
_RANK = {"NONE": 0, INTRON: 1, EXON: 2}                  # GtfRecord::RecordType (GtfRecord.h:20-26)
HAS_NOT_ANNOTATED, HAS_EXONS, HAS_INTRONS = 1, 2, 4      # UMI::Mark (UMI.h:16-22)
_BIT = {EXON: HAS_EXONS, INTRON: HAS_INTRONS}            # Mark::add(RecordType) (UMI.cpp:87-100)
CLASSES = ("both_empty", "one_one_same", "one_one_differ", "half_annotated", "empty_vs_many", "many_find_exon_fails",
           "many_exons_agree", "many_exons_differ", "many_one_side_intron_only")


def ordered(results):
    """(gene, type) pairs as std::set<QueryResult> holds them: by type, then by name (RefGenesContainer.cpp:255-261)"""
    return sorted(set(results), key=lambda r: (_RANK[r[1]], r[0]))


def _find_exon(results):
    """ReadParamsParser::find_exon (:153-172) -> (ok, gene of the first exon or "")"""
    exon = ""
    for gene, type_ in results:
        if type_ != EXON:
            continue
        if exon == "":
            exon = gene
            continue
        if exon != gene:
            return False, exon
    return True, exon


def decide(set1, set2):
    """get_gene_from_reference (:92-151) -> (gene or "", mark bits)"""
    set1, set2 = ordered(set1), ordered(set2)
    if not set1 and not set2:                                             # :102-103
        return "", 0
    if len(set1) == 1 and len(set2) == 1:                                 # :105-116
        if set1[0][0] == set2[0][0]:
            return set1[0][0], _BIT[set1[0][1]] | _BIT[set2[0][1]]
        return "", 0
    if len(set1) <= 1 and len(set2) <= 1:                                 # :118-126
        gene, type_ = set2[0] if not set1 else set1[0]
        return gene, _BIT[type_] | HAS_NOT_ANNOTATED
    if not set1 or not set2:                                              # :128-129
        return "", 0
    ok1, exon1 = _find_exon(set1)                                         # :131-136
    if not ok1:
        return "", 0
    ok2, exon2 = _find_exon(set2)
    if not ok2:
        return "", 0
    if exon1 != "" and exon2 != "":                                       # :138-148
        if exon1 != exon2:
            return "", 0
        return exon1, HAS_EXONS
    return "", 0                                                          # :150


def classify(set1, set2):
    set1, set2 = ordered(set1), ordered(set2)
    n1, n2 = len(set1), len(set2)
    if n1 == 0 and n2 == 0:
        return "both_empty"
    if n1 == 1 and n2 == 1:
        return "one_one_same" if set1[0][0] == set2[0][0] else "one_one_differ"
    if n1 <= 1 and n2 <= 1:
        return "half_annotated"
    if n1 == 0 or n2 == 0:
        return "empty_vs_many"
    (ok1, exon1), (ok2, exon2) = _find_exon(set1), _find_exon(set2)
    if not ok1 or not ok2:
        return "many_find_exon_fails"
    if exon1 != "" and exon2 != "":
        return "many_exons_agree" if exon1 == exon2 else "many_exons_differ"
    return "many_one_side_intron_only"


class Record:
    __slots__ = ("chr", "type", "start", "end", "gene", "transcript")

    def __init__(self, chr_, type_, start, end, gene, transcript):
        self.chr, self.type, self.start, self.end, self.gene, self.transcript = chr_, type_, start, end, gene, transcript


def read_gtf(path):
    """The exon / intron records of a GTF as RefGenesContainer::parse_gtf_record keeps them (:116-180): the name is
    gene_name if there is one, else gene_id (GtfRecord::gene_name); the transcript is transcript_id, else gene_id."""
    out = []
    with (gzip.open(path, "rt") if path.endswith(".gz") else open(path)) as f:
        for line in f:
            col = line.split()
            if not col or line[0] == "#" or len(col) <= 9 or col[2] not in ("exon", "intron"):
                continue
            attr = {col[a]: col[a + 1][1:-2] for a in range(8, len(col) - 1)}
            gene_id = attr.get("gene_id") or attr.get("gene_name")
            out.append(Record(col[0], EXON if col[2] == "exon" else INTRON, int(col[3]) - 1, int(col[4]),
                              attr.get("gene_name") or gene_id, attr.get("transcript_id") or gene_id))
    return out


class _Transcript:
    def __init__(self, gene):
        self.gene, self.start, self.end, self.exons, self.introns = gene, None, None, [], []


class Annotation:
    def __init__(self, records):
        self.chromosomes = {}                     # name -> {transcript id -> _Transcript}
        self.use_introns = any(r.type == INTRON for r in records)          # _use_introns_from_gtf (:134-138)
        for r in records:
            t = self.chromosomes.setdefault(r.chr, {}).setdefault(r.transcript, _Transcript(r.gene))
            assert t.gene == r.gene
            t.start = r.start if t.start is None else min(t.start, r.start)
            t.end = r.end if t.end is None else max(t.end, r.end)
            (t.exons if r.type == EXON else t.introns).append((r.start, r.end))
        self._memo = {}

    def is_simple(self):
        ids = [tid for c in self.chromosomes.values() for tid in c]
        if len(ids) != len(set(ids)):
            return False
        for c in self.chromosomes.values():
            for t in c.values():
                spans = sorted(t.exons + t.introns)
                if any(a[1] > b[0] for a, b in zip(spans, spans[1:])) or any(s >= e for s, e in spans):
                    return False
        return True

    def query(self, chr_, start, end):
        """get_gene_info(chr, start, end) (:182-213) -> ordered [(gene, type)], None for an unknown chromosome"""
        if end < start:                                                   # :185-186
            return []
        if chr_ not in self.chromosomes:                                  # :188-190
            return None
        key = (chr_, start, end)
        if key not in self._memo:
            results = []
            for t in self.chromosomes[chr_].values():
                if not (t.start < end and t.end > start):
                    continue
                ex = any(s < end and e > start for s, e in t.exons)
                in_ = any(s < end and e > start for s, e in t.introns)
                if not ex and not in_:
                    if not self.use_introns:                              # :201-205
                        results.append((t.gene, INTRON))
                    continue
                if ex:
                    results.append((t.gene, EXON))
                if in_:
                    results.append((t.gene, INTRON))
            self._memo[key] = ordered(results)
        return self._memo[key]

    def depth(self, chr_, p):
        """distinct transcripts whose extent covers p"""
        key = (chr_, p)
        if key not in self._memo:
            self._memo[key] = sum(1 for t in self.chromosomes.get(chr_, {}).values() if t.start <= p < t.end)
        return self._memo[key]

    def sets_of_read(self, chr_, position, end_position):
        """the two result sets of a read (ReadParamsParser.cpp:98-100); end_position - 1 of 0 wraps round in the
        reference's size_t, which get_gene_info answers with the empty set (:185-186)"""
        if chr_ not in self.chromosomes:
            return None
        return self.query(chr_, position, position + 1), (self.query(chr_, end_position - 1, end_position) if end_position >= 1 else [])

    def depths_of_read(self, chr_, position, end_position):
        return self.depth(chr_, position), (self.depth(chr_, end_position - 1) if end_position >= 1 else 0)

    def gene_for_read(self, chr_, position, end_position):
        sets = self.sets_of_read(chr_, position, end_position)
        return None if sets is None else decide(*sets)

    def class_of_read(self, chr_, position, end_position):
        sets = self.sets_of_read(chr_, position, end_position)
        return "unknown_chromosome" if sets is None else classify(*sets)
