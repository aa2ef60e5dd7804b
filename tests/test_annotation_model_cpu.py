"""The plain model of the reference's read annotation (annotation_model.py) against the oracle, the host product against the
oracle on the generated files (annotation_cases.py), and the conditions the dense query stream must meet so that the device
test (test_gpu_annotation.py) cannot pass on an easy stream.  Host-only: runs without a GPU.  Every comparison is exact."""
import collections

import pytest

import annotation_cases as ac
import annotation_model as am
from oracle import binding as ob

from test_gene_annotation import GTF, Product

CAP = 16      # what the kernel holds per end point (ANN_CAP, csrc/annotation_api.hip)


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    d = tmp_path_factory.mktemp("annotation_cases")
    return {s: ac.make(d, s) for s in ac.STREAMS}


def test_model_on_the_reference_known_answers():
    """testGenesWithIntrons (Tests/TestTools.cpp:266-287), the values of test_oracle_reference_kat.py.  (The reference's GTF is not a
    simple file in the model's sense -- three of its transcripts carry overlapping records -- so no more than these is claimed on it.)"""
    m = am.Annotation(am.read_gtf(GTF))
    assert not m.is_simple()
    assert m.query("chr1", 20000, 20010) == [("WASH7P", "INTRON")]
    assert m.query("chr1", 24750, 24760) == [("WASH7P", "EXON")]
    assert m.query("chr1", 10, 20) == [] and m.query("chrNope", 10, 20) is None
    assert m.gene_for_read("chr1", 24750, 24800) == ("WASH7P", 2) and m.gene_for_read("chrNope", 1, 50) is None


def test_decide_branch_by_branch():
    E, I = am.EXON, am.INTRON
    assert am.decide([], []) == ("", 0)
    assert am.decide([("A", E)], [("A", I)]) == ("A", 6) and am.decide([("A", E)], [("B", E)]) == ("", 0)
    assert am.decide([], [("A", I)]) == ("A", 5) and am.decide([("A", E)], []) == ("A", 3)
    assert am.decide([], [("A", E), ("B", E)]) == ("", 0)
    assert am.decide([("A", E), ("B", I)], [("A", E)]) == ("A", 2)
    assert am.decide([("A", E), ("B", I)], [("B", E), ("A", I)]) == ("", 0)
    assert am.decide([("A", E), ("B", E)], [("A", E)]) == ("", 0)
    assert am.decide([("A", I), ("B", I)], [("A", E)]) == ("", 0)
    assert am.ordered([("B", E), ("A", E), ("Z", I), ("A", E)]) == [("Z", I), ("A", E), ("B", E)]
    assert am.classify([("A", E), ("A", I)], [("A", E)]) == "many_exons_agree"
    assert am.classify([("A", I), ("B", I)], [("A", E)]) == "many_one_side_intron_only"


@pytest.mark.parametrize("stream", ac.STREAMS)
def test_model_and_host_product_equal_the_oracle(cases, stream):
    """model == oracle on every query of every simple file (result sets of both end points and the read's gene and mark);
    host product == oracle on all files, BED included"""
    case = cases[stream]
    assert case.model.is_simple() == case.simple
    o, p = ob.GeneAnnotationOracle(case.path), Product(case.path)
    points = set()
    for chr_, pos, end in case.queries:
        want = o.gene_for_read(chr_, pos, end)
        got = p.gene_for_read(chr_, pos, end)
        assert got == want, ("host product", chr_, pos, end, got, want)
        if case.simple:
            got = case.model.gene_for_read(chr_, pos, end)
            assert got == want, ("model", chr_, pos, end, got, want, case.model.depths_of_read(chr_, pos, end), case.model.class_of_read(chr_, pos, end))
        points.update(((chr_, pos), (chr_, end - 1)) if end >= 1 else ((chr_, pos),))
    for chr_, x in points:
        want = o.query(chr_, x, x + 1)
        assert p.query(chr_, x, x + 1) == want, ("host product", chr_, x)
        if case.simple:
            assert case.model.query(chr_, x, x + 1) == want, ("model", chr_, x)
    # spans longer than a base (get_gene_info as the reference's own tests call it)
    for chr_, pos, end in case.queries[::17]:
        if 1 < end - pos <= 40 and not (case.simple and len(case.model.query(chr_, pos, end) or []) > 60):      # (the bindings hold 64 results)
            want = o.query(chr_, pos, end)
            if want is not None:
                assert p.query(chr_, pos, end) == want, ("host product", chr_, pos, end)
                if case.simple:
                    assert case.model.query(chr_, pos, end) == want, ("model", chr_, pos, end)


def _depth_report(case):
    m = case.model
    classes, hist = collections.Counter(), collections.Counter()
    deep = deep_one = deep_many = mid = exactly_cap = 0
    for chr_, pos, end in case.queries:
        sets = m.sets_of_read(chr_, pos, end)
        if sets is None:
            continue
        classes[am.classify(*sets)] += 1
        depths = m.depths_of_read(chr_, pos, end)
        hist[max(depths)] += 1
        over = [len(s) for s, d in zip(sets, depths) if d > CAP]
        deep += bool(over)
        deep_one += any(n == 1 for n in over)
        deep_many += any(n > CAP for n in over)
        mid += any(9 <= d <= CAP for d in depths)
        exactly_cap += any(d == CAP for d in depths)
    return classes, hist, dict(deep=deep, deep_one=deep_one, deep_many=deep_many, mid=mid, exactly_cap=exactly_cap)


@pytest.mark.parametrize("stream", ["dense", "dense_introns"])
def test_dense_stream_reaches_every_branch_and_the_capacity(cases, stream):
    """Asserted on the model alone: what the dense stream must contain for the device test to mean something."""
    case = cases[stream]
    classes, hist, n = _depth_report(case)
    print(stream, "queries", len(case.queries), "classes", dict(classes), "depth histogram (larger end point)", sorted(hist.items()), n)
    for c in am.CLASSES:
        assert classes[c] >= 100, (c, classes[c])
    assert n["deep"] >= 500 and n["deep_one"] >= 100 and n["deep_many"] >= 100, n
    assert n["mid"] >= 1000 and n["exactly_cap"] >= 1, n
    # every boundary of the file with its triples, worked out again from the records
    have = set(case.queries)
    n_bounds = 0
    for r_chr in case.chromosomes:
        bs = sorted({x for r in case.records if r.chr == r_chr for x in (r.start, r.end)})
        n_bounds += len(bs)
        for i, b in enumerate(bs):
            for p in (b - 1, b, b + 1):
                for b2 in bs[i + 1:i + 1 + ac.K_NEXT]:
                    for e in (b2 - 1, b2, b2 + 1):
                        assert p < 0 or (r_chr, p, e) in have, (r_chr, p, e)
    assert n_bounds > 500
    assert any(e == 0 for _, _, e in case.queries) and any(p == e for _, p, e in case.queries) and any(c == "chrNope" for c, _, _ in case.queries)


@pytest.mark.parametrize("stream", ["sparse", "far", "bed"])
def test_the_other_streams_stay_below_the_capacity(cases, stream):
    case = cases[stream]
    assert all(max(case.model.depths_of_read(*q)) <= CAP for q in case.queries)
    if stream == "far":
        assert max(r.end for r in case.records) == ac.FAR_TOP and any(p >= ac.FAR_TOP - 1 for _, p, _ in case.queries)
        assert ("chrZero", 0, 1) in case.queries and case.model.gene_for_read("chrZero", 0, 1) == ("GZero", 2)
        assert case.model.gene_for_read("chrZero", 0, 0) == ("GZero", 3) and case.model.gene_for_read("chrZero", 1, 2) == ("", 0)
