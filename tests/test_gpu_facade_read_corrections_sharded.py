"""`dropest -F`, the decisions, through the C++ facade on one device and on a sharded container: tests/cpp/read_corrections_dump on the
whitelist and N-UMI streams of test_gpu_read_corrections.py.  Devices "0", "0,0" and "0,0,0" give the same verdict, target barcode code and
corrected UMI code for every read, and what they give is what tests/filtered_model.py makes of the oracle's state."""
import subprocess

import numpy as np
import pytest

import filtered_model as fm
from dropest_amd import capi
from dropest_amd.build import CORRECTIONS_TOOL, build_facade
from oracle import Oracle
from test_gpu_read_corrections import BASE_O, Stream, _final_molecules

pytestmark = pytest.mark.gpu

CASES = {"whitelist": dict(seed=2, children=3), "n_umis": dict(seed=7, n_umis=150)}


def dump(devices, records, whitelist, out):
    r = subprocess.run([CORRECTIONS_TOOL, devices, str(records), whitelist or "-", str(BASE_O["min_genes_before"]), str(BASE_O["min_genes_after"]), str(out)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "shards %d" % len(devices.split(",")) in r.stdout
    return np.loadtxt(str(out), dtype=np.uint64, ndmin=2)


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_lists_give_identical_dumps(name, tmp_path):
    build_facade()
    s = Stream(**CASES[name])
    whitelist = s.write_whitelist(tmp_path) if name == "whitelist" else None
    records = tmp_path / "records.txt"
    barcode = [capi.unpack_code(x, s.side) for x in s.cb]
    records.write_text("".join("%s %s %s\n" % (b, u, "-" if g == capi.NO_GENE else "Gene%d" % g) for b, u, g in zip(barcode, s.umi_text, s.gene)))
    one = dump("0", records, whitelist, tmp_path / "one.txt")
    assert np.array_equal(dump("0,0", records, whitelist, tmp_path / "two.txt"), one)
    assert np.array_equal(dump("0,0,0", records, whitelist, tmp_path / "three.txt"), one)
    # the verdicts are the model's on the oracle's state (the facade numbers genes and packs UMIs in its own way: verdicts and barcodes only)
    okw = dict(BASE_O, merge_kind=1, barcodes_kind=1, barcodes_file=whitelist) if whitelist else dict(BASE_O)
    o = Oracle(**okw); o.add_packed(s.cb, s.umi, s.gene, s.aux, s.side); o.set_initialized(); o.merge_and_filter()
    cbs = fm.merge_cbs(o.merge_targets(), o.filtered_cells())
    mols = _final_molecules(o)
    want = []
    for cell, g, u in zip(s.cell, s.gene, s.umi_text):
        v = fm.decide_read(int(cell), None if g == capi.NO_GENE else int(g), u, cbs, mols, {})[0]
        want.append(fm.WRITTEN if v == fm.WRONG_UMI else v)          # the targets are kept: both strategies hand out final targets
    assert one[:, 0].tolist() == want and want.count(fm.WRITTEN) * 4 >= len(want)
    first_of = {int(c): i for i, c in reversed(list(enumerate(s.cell)))}
    for i in range(len(want)):
        target = cbs.get(int(s.cell[i])) if s.gene[i] != capi.NO_GENE else None
        assert int(one[i, 1]) == (0 if target is None else capi.pack_seq(barcode[first_of[target]]))
