"""`dropest -S` through the C++ facade: tests/cpp/validation_to_rds on the planted case of validation_cases.py.  The .rds carries
merge_validation_info = list(distant, adjacent), each with the reference's six names in its order (ResultsPrinter.cpp:476-509) as real
vectors; the values are the C-ABI call's on a context fed the same reads; without validation_stats the list is today's."""
import subprocess

import numpy as np
import pytest

from dropest_amd import capi
from dropest_amd.build import VALIDATION_TOOL, build_facade

import rds_reader
import validation_cases as vc

pytestmark = pytest.mark.gpu

NAMES = ["Probability", "UmisPerCell1", "UmisPerCell2", "EditDistance", "IntersectionSize", "ExpectedIntersectionSize"]
KEYS = ["probability", "umis1", "umis2", "edit_distance", "intersection", "expected"]
TODAY = ["cm", "cm_raw", "reads_per_chr_per_cells", "mean_reads_per_umi", "saturation_info", "merge_targets", "aligned_reads_per_cell",
         "aligned_umis_per_cell", "requested_umis_per_cb", "requested_reads_per_cb"]
N_DISTANT, N_ADJACENT, MAX_DRAWS = 200, 64, 1 << 16


@pytest.fixture(scope="module")
def records(tmp_path_factory):
    build_facade()
    c = vc.case("planted")
    path = tmp_path_factory.mktemp("validation_facade") / "records.txt"
    lines = []
    for cell, gene, umi, reads in c.molecules:
        lines += ["%s %s Gene%d" % (c.barcodes[cell], umi, gene)] * reads
    path.write_text("\n".join(lines) + "\n")
    return c, path


def run_tool(path, out, stats, adjacent=N_ADJACENT, max_draws=MAX_DRAWS):
    r = subprocess.run([VALIDATION_TOOL, str(path), str(out), str(int(stats)), str(N_DISTANT), str(adjacent), str(max_draws), "1"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return rds_reader.read_rds(str(out)), r.stdout


def test_rds_carries_both_samples_with_the_c_abi_values(records, tmp_path):
    c, path = records
    d, stdout = run_tool(path, tmp_path / "with.rds", True)
    assert "truncated 0" in stdout
    assert d.names == TODAY + ["merge_validation_info"]
    info = d["merge_validation_info"]
    assert info.kind == "list" and len(info.value) == 2 and info.names is None
    # the same reads through the C-ABI: one gene-bearing read per line of the file, cells numbered as they first appear
    # and genes: an estimate is a sum over the common genes in gene-id order, so the ids have to be the facade's for equal bits
    gene_id = {}
    cb, umi, gene = [], [], []
    side = []

    def code(text):
        k = capi.pack_seq(text)
        if k is None:
            if text not in side:
                side.append(text)
            k = capi.ESCAPE | side.index(text)
        return k

    for cell, g, u, reads in c.molecules:
        for _ in range(reads):
            cb.append(code(c.barcodes[cell])); umi.append(code(u)); gene.append(gene_id.setdefault(g, len(gene_id)))
    ctx = capi.Context(**c.ctx)
    try:
        ctx.set_side_strings(side)
        ctx.push_reads(np.array(cb, np.uint64), np.array(umi, np.uint64), np.array(gene, np.uint32), np.full(len(cb), 2 << 16, np.uint32))
        ctx.set_initialized()
        ctx.merge_and_filter()
        want = ctx.merge_validation((5, 100, N_DISTANT), (1, 1, N_ADJACENT), max_draws=MAX_DRAWS)
    finally:
        ctx.close()
    for sample, w, n in zip(info.value, want, (N_DISTANT, N_ADJACENT)):
        assert sample.kind == "list" and sample.names == NAMES
        assert w["n_found"] == n
        for name, key in zip(NAMES, KEYS):
            v = sample[name]
            assert v.kind == "double" and len(v.value) == n, name
            assert np.array_equal(v.value, w[key].astype(np.float64)), name


def test_without_validation_stats_the_list_is_todays(records, tmp_path):
    _, path = records
    d, _ = run_tool(path, tmp_path / "without.rds", False)
    assert d.names == TODAY


def test_a_truncated_sample_is_written_with_what_it_found(records, tmp_path):
    _, path = records
    d, stdout = run_tool(path, tmp_path / "short.rds", True, adjacent=4000, max_draws=5000)
    assert "truncated 1" in stdout
    distant, adjacent = d["merge_validation_info"].value
    assert len(distant["Probability"].value) == N_DISTANT
    assert 0 < len(adjacent["Probability"].value) < 4000
    assert all(len(adjacent[n].value) == len(adjacent["Probability"].value) for n in NAMES)
