"""dropest_bam_decoder_filter_window_segments without a GPU: the library exports it, the header declares the segment as the tests' ctypes mirror
lays it out, and a call without a decoder is refused before anything touches a device (tests/test_gpu_bam_filter_segments.py has the rest)."""
import ctypes as C
import os
import re

from dropest_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Segment(C.Structure):
    _fields_ = [("count", C.c_uint64), ("verdict", C.c_void_p), ("cell", C.c_void_p), ("umi", C.c_void_p), ("device", C.c_int32)]


def test_the_call_is_exported_and_declared():
    L = capi.lib()
    assert hasattr(L, "dropest_bam_decoder_filter_window_segments"), "missing export"
    header = open(os.path.join(ROOT, "include", "dropest_bgzf.h")).read()
    m = re.search(r"typedef struct dropest_bam_decision_segment \{(.*?)\} dropest_bam_decision_segment;", header, re.S)
    assert m, "the header does not declare the segment"
    fields = [(t.strip(), n) for t, n in re.findall(r"^\s*(?:const )?(\w+) \*?(\w+);", m.group(1), re.M)]
    assert fields == [("uint64_t", "count"), ("uint8_t", "verdict"), ("uint32_t", "cell"), ("uint64_t", "umi"), ("int32_t", "device")]
    assert [n for n, _ in Segment._fields_] == [n for _, n in fields] and C.sizeof(Segment) == 40


def test_a_call_without_a_decoder_is_refused():
    L = capi.lib()
    L.dropest_bgzf_last_error.restype = C.c_char_p
    L.dropest_bam_decoder_filter_window_segments.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    ptr, ln, nw = C.c_void_p(), C.c_uint64(7), C.c_uint64(7)
    seg = Segment(0, None, None, None, 0)
    assert L.dropest_bam_decoder_filter_window_segments(None, C.byref(seg), 1, C.byref(ptr), C.byref(ln), C.byref(nw)) == 1
    assert b"null argument" in L.dropest_bgzf_last_error()
