"""`dropest -S` through the C++ facade on a SHARDED container: tests/cpp/validation_sharded_to_rds with three shards on device 0 on the
planted records of test_gpu_validation_facade.py.  merge_validation_info stands where one context's stands, with the reference's six
names in its order as real vectors, and its values are bit-equal to validation_to_rds's .rds on the same file; without validation_stats
the list is today's."""
import subprocess

import numpy as np
import pytest

from dropest_amd.build import VALIDATION_SHARDED_TOOL, VALIDATION_TOOL, build_facade

import rds_reader
import validation_cases as vc
from test_gpu_validation_facade import MAX_DRAWS, N_ADJACENT, N_DISTANT, NAMES, TODAY

pytestmark = pytest.mark.gpu

DEVICES = "0,0,0"


@pytest.fixture(scope="module")
def records(tmp_path_factory):
    build_facade()
    c = vc.case("planted")
    path = tmp_path_factory.mktemp("validation_sharded_facade") / "records.txt"
    lines = []
    for cell, gene, umi, reads in c.molecules:
        lines += ["%s %s Gene%d" % (c.barcodes[cell], umi, gene)] * reads
    path.write_text("\n".join(lines) + "\n")
    return path


def run(tool, lead, path, out, stats):
    r = subprocess.run([tool] + lead + [str(path), str(out), str(int(stats)), str(N_DISTANT), str(N_ADJACENT), str(MAX_DRAWS), "1"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return rds_reader.read_rds(str(out)), r.stdout


def test_sharded_rds_equals_one_contexts(records, tmp_path):
    d, stdout = run(VALIDATION_SHARDED_TOOL, [DEVICES], records, tmp_path / "sharded.rds", True)
    assert "truncated 0" in stdout and "shards 3" in stdout
    one, _ = run(VALIDATION_TOOL, [], records, tmp_path / "one.rds", True)
    assert d.names == TODAY + ["merge_validation_info"] == one.names
    info, want = d["merge_validation_info"], one["merge_validation_info"]
    assert info.kind == "list" and len(info.value) == 2 and info.names is None
    for sample, ref, n in zip(info.value, want.value, (N_DISTANT, N_ADJACENT)):
        assert sample.kind == "list" and sample.names == NAMES
        for name in NAMES:
            v = sample[name]
            assert v.kind == "double" and len(v.value) == n, name
            assert np.asarray(v.value, np.float64).tobytes() == np.asarray(ref[name].value, np.float64).tobytes(), name
    assert any(x > 0 for x in info.value[1]["IntersectionSize"].value)


def test_without_validation_stats_the_list_is_todays(records, tmp_path):
    d, _ = run(VALIDATION_SHARDED_TOOL, [DEVICES], records, tmp_path / "without.rds", False)
    assert d.names == TODAY
