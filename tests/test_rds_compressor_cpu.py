"""Rds::save through a compressor object (dropest_amd/csrc/host/rds_writer.h: Rds::Compressor): the hook a device compressor is injected
through, checked on the host alone.  rds_writer.cpp is compiled on its own, as tests/test_rds.py does; the long-vector value of
tests/cpp/test_rds_writer.cpp is saved by the default writer and through a compressor that cuts every piece into zlib members of at most
65 280 bytes, in batches of three pieces: both files must hold the same serialisation byte for byte and parse to the same tree, and the
default compressor object must write the default writer's bytes."""
import os
import struct
import subprocess
import zlib

import numpy as np

import rds_reader as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same_tree(a, b):
    assert a.kind == b.kind and a.is_object == b.is_object and list(a.attributes) == list(b.attributes)
    for k in a.attributes:
        same_tree(a.attributes[k], b.attributes[k])
    if a.kind == "list":
        assert len(a.value) == len(b.value)
        for x, y in zip(a.value, b.value):
            same_tree(x, y)
    elif isinstance(a.value, np.ndarray):
        assert np.array_equal(a.value, b.value, equal_nan=a.value.dtype.kind == "f")
    else:
        assert a.value == b.value


def test_compressor_overload_writes_the_same_serialisation(tmp_path):
    exe = str(tmp_path / "c")
    src = [os.path.join(ROOT, "tests", "cpp", "test_rds_compressor.cpp"), os.path.join(ROOT, "dropest_amd", "csrc", "host", "rds_writer.cpp")]
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall"] + src + ["-o", exe, "-lz", "-pthread"])
    plain, chunked = str(tmp_path / "plain.rds"), str(tmp_path / "chunked.rds")
    out = subprocess.run([exe, plain, chunked, str(6 << 20)], capture_output=True, text=True).stdout.split()
    assert out and out[0] == "ok", out
    calls, pieces = int(out[1].split("=")[1]), int(out[2].split("=")[1])
    assert calls >= 3 and pieces > 2 * calls                       # several batches of three pieces (the last may be short)
    raw_plain, raw_chunked = open(plain, "rb").read(), open(chunked, "rb").read()
    assert open(chunked + ".host", "rb").read() == raw_plain        # the default compressor object = the default writer
    data = rr.decompress(raw_plain)
    assert rr.decompress(raw_chunked) == data
    members, rest = 0, raw_chunked                                  # every member holds at most 65 280 bytes
    while rest:
        z = zlib.decompressobj(31)
        assert len(z.decompress(rest)) <= 65_280 and z.eof
        rest = z.unused_data
        members += 1
    assert members >= len(data) // 65_280
    same_tree(rr.read_rds(plain), rr.read_rds(chunked))
