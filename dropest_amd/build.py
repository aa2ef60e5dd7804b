"""Builds dropest_amd/lib/libdropest_amd.so with hipcc for gfx950 (in-tree, so it travels to the GPU box)."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB_DIR = os.path.join(HERE, "lib")
LIB = os.path.join(LIB_DIR, "libdropest_amd.so")
SOURCES = ["dropest_amd.hip", "synth_api.hip", "annotation_api.hip", "bgzf_api.hip", "deflate_api.hip"]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wall", "-Wno-unused-function", "-pthread"]
OBJ_DIR = os.path.join(LIB_DIR, "obj")


def _hipcc():
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found")


def _deps_of(src):
    """What the object of `src` was built from: the compiler's own list (hipcc -MMD writes obj/<name>.d beside the object; ADVICE r5: a hand-kept
    list went stale).  Without one: every file under csrc/ and include/."""
    dep = os.path.join(OBJ_DIR, src.replace(".hip", ".d"))
    if os.path.exists(dep):
        words = open(dep).read().replace("\\\n", " ").split()
        files = [w for w in words[1:] if not w.endswith(":") and not w.startswith("/opt/")]
        if files and all(os.path.exists(f) for f in files):
            return files
    inc = os.path.join(HERE, "..", "include")
    return [os.path.join(CSRC, f) for f in os.listdir(CSRC) if not f.endswith(".hip") or f == src] + [os.path.join(inc, f) for f in os.listdir(inc)]


def _stale():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    deps = [os.path.join(CSRC, f) for f in os.listdir(CSRC)]
    deps += [os.path.join(HERE, "..", "include", f) for f in os.listdir(os.path.join(HERE, "..", "include"))]
    return any(os.path.isfile(d) and os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=False):
    """Compile every HIP source of the package (one object per source, rebuilt when the source or a header it uses changed, or all of
    them with force) and link them into one shared library.  Returns its path."""
    if not force and not _stale():
        return LIB
    os.makedirs(OBJ_DIR, exist_ok=True)
    extra = os.environ.get("DROPEST_EXTRA_HIPCC_FLAGS", "").split()
    objs, procs = [], []
    for s in SOURCES:
        obj = os.path.join(OBJ_DIR, s.replace(".hip", ".o"))
        objs.append(obj)
        if not force and not extra and os.path.exists(obj) and all(os.path.getmtime(d) <= os.path.getmtime(obj) for d in _deps_of(s)):
            continue
        cmd = [_hipcc()] + FLAGS + extra + ["-MMD", "-MF", obj[:-2] + ".d", "-c", os.path.join(CSRC, s), "-o", obj]
        if verbose:
            print(" ".join(cmd))
        procs.append((cmd, subprocess.Popen(cmd)))
    for cmd, p in procs:
        if p.wait():
            raise subprocess.CalledProcessError(p.returncode, cmd)
    cmd = [_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-pthread"] + objs + ["-o", LIB]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return LIB


FACADE_LIB = os.path.join(LIB_DIR, "libdropest_facade.so")
FACADE_TEST = os.path.join(HERE, "..", "tests", "cpp", "test_facade")
BAM_TOOL = os.path.join(HERE, "..", "tests", "cpp", "bam_to_counts")
RATE_TOOL = os.path.join(HERE, "..", "tests", "cpp", "add_record_rate")
RDS_TOOL = os.path.join(HERE, "..", "tests", "cpp", "bam_to_rds")
SHARDED_BAM_TOOL = os.path.join(HERE, "..", "tests", "cpp", "bam_sharded_device")
VALIDATION_TOOL = os.path.join(HERE, "..", "tests", "cpp", "validation_to_rds")
VALIDATION_SHARDED_TOOL = os.path.join(HERE, "..", "tests", "cpp", "validation_sharded_to_rds")
TAGGED_TOOL = os.path.join(HERE, "..", "tests", "cpp", "bam_tagged")
UMI_TARGETS_TOOL = os.path.join(HERE, "..", "tests", "cpp", "umi_merge_targets")
FILTERED_TOOL = os.path.join(HERE, "..", "tests", "cpp", "bam_filtered")
FILTERED_SHARDED_TOOL = os.path.join(HERE, "..", "tests", "cpp", "bam_filtered_sharded")
CORRECTIONS_TOOL = os.path.join(HERE, "..", "tests", "cpp", "read_corrections_dump")
SOURCES_TOOL = os.path.join(HERE, "..", "tests", "cpp", "bam_sources")
SOURCES_OUTPUT_TOOL = os.path.join(HERE, "..", "tests", "cpp", "bam_sources_output")


def build_facade(force=False, verbose=False):
    """g++: the C++ facade (host/facade.cpp, plain host code over the C-ABI) and the reference-style test driver."""
    build(force=False)
    src = os.path.join(CSRC, "host", "facade.cpp")
    rds = os.path.join(CSRC, "host", "rds_writer.cpp")
    bam = os.path.join(CSRC, "host", "bam_ingest.cpp")
    bam_ctl = os.path.join(CSRC, "host", "bam_controller.cpp")
    bam_dev = os.path.join(CSRC, "host", "bam_device.cpp")
    ga = os.path.join(CSRC, "host", "gene_annotation.cpp")
    hdr = os.path.join(CSRC, "host", "facade.h")
    test_src = os.path.join(HERE, "..", "tests", "cpp", "test_facade.cpp")
    bam_tool_src = os.path.join(HERE, "..", "tests", "cpp", "bam_to_counts.cpp")
    rate_src = os.path.join(HERE, "..", "tests", "cpp", "add_record_rate.cpp")
    rds_tool_src = os.path.join(HERE, "..", "tests", "cpp", "bam_to_rds.cpp")
    sharded_bam_src = os.path.join(HERE, "..", "tests", "cpp", "bam_sharded_device.cpp")
    validation_src = os.path.join(HERE, "..", "tests", "cpp", "validation_to_rds.cpp")
    validation_sharded_src = os.path.join(HERE, "..", "tests", "cpp", "validation_sharded_to_rds.cpp")
    tagged_src = os.path.join(HERE, "..", "tests", "cpp", "bam_tagged.cpp")
    umi_targets_src = os.path.join(HERE, "..", "tests", "cpp", "umi_merge_targets.cpp")
    filtered_src = os.path.join(HERE, "..", "tests", "cpp", "bam_filtered.cpp")
    filtered_sharded_src = os.path.join(HERE, "..", "tests", "cpp", "bam_filtered_sharded.cpp")
    corrections_src = os.path.join(HERE, "..", "tests", "cpp", "read_corrections_dump.cpp")
    sources_src = os.path.join(HERE, "..", "tests", "cpp", "bam_sources.cpp")
    sources_output_src = os.path.join(HERE, "..", "tests", "cpp", "bam_sources_output.cpp")
    newest = max(os.path.getmtime(x) for x in (src, rds, bam, bam_ctl, bam_dev, ga, os.path.join(CSRC, "host", "rds_writer.h"), os.path.join(CSRC, "host", "bam_ingest.h"),
                                               os.path.join(CSRC, "host", "bam_parse.h"), os.path.join(CSRC, "host", "bgzf_blocks.h"),
                                               os.path.join(CSRC, "host", "gene_annotation.h"),
                                               hdr, test_src, bam_tool_src, rate_src, rds_tool_src, sharded_bam_src, validation_src, validation_sharded_src, tagged_src, umi_targets_src, filtered_src, filtered_sharded_src, corrections_src, sources_src, sources_output_src, LIB))
    if not force and os.path.exists(FACADE_LIB) and os.path.exists(FACADE_TEST) and os.path.exists(BAM_TOOL) and os.path.exists(RATE_TOOL) and os.path.exists(RDS_TOOL) and \
            os.path.exists(SHARDED_BAM_TOOL) and os.path.exists(VALIDATION_TOOL) and os.path.exists(VALIDATION_SHARDED_TOOL) and os.path.exists(TAGGED_TOOL) and os.path.exists(UMI_TARGETS_TOOL) and os.path.exists(FILTERED_TOOL) and os.path.exists(FILTERED_SHARDED_TOOL) and os.path.exists(CORRECTIONS_TOOL) and os.path.exists(SOURCES_TOOL) and os.path.exists(SOURCES_OUTPUT_TOOL) and \
            min(os.path.getmtime(FACADE_LIB), os.path.getmtime(FACADE_TEST), os.path.getmtime(BAM_TOOL), os.path.getmtime(RATE_TOOL), os.path.getmtime(RDS_TOOL),
                os.path.getmtime(SHARDED_BAM_TOOL), os.path.getmtime(VALIDATION_TOOL), os.path.getmtime(VALIDATION_SHARDED_TOOL), os.path.getmtime(TAGGED_TOOL), os.path.getmtime(UMI_TARGETS_TOOL), os.path.getmtime(FILTERED_TOOL), os.path.getmtime(FILTERED_SHARDED_TOOL), os.path.getmtime(CORRECTIONS_TOOL), os.path.getmtime(SOURCES_TOOL), os.path.getmtime(SOURCES_OUTPUT_TOOL)) > newest:
        return FACADE_LIB, FACADE_TEST
    cmds = [
        ["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", src, rds, bam, bam_ctl, bam_dev, ga, "-o", FACADE_LIB, "-L" + LIB_DIR, "-ldropest_amd", "-lz",
         "-lpthread", "-Wl,-rpath,$ORIGIN"],
        ["g++", "-O2", "-std=c++17", "-Wall", test_src, "-o", FACADE_TEST, "-L" + LIB_DIR, "-ldropest_facade", "-ldropest_amd",
         "-Wl,-rpath,$ORIGIN/../../dropest_amd/lib"],
        ["g++", "-O2", "-std=c++17", "-Wall", bam_tool_src, "-o", BAM_TOOL, "-L" + LIB_DIR, "-ldropest_facade", "-ldropest_amd",
         "-Wl,-rpath,$ORIGIN/../../dropest_amd/lib"],
        ["g++", "-O2", "-std=c++17", "-Wall", rate_src, "-o", RATE_TOOL, "-L" + LIB_DIR, "-ldropest_facade", "-ldropest_amd",
         "-Wl,-rpath,$ORIGIN/../../dropest_amd/lib"],
        ["g++", "-O2", "-std=c++17", "-Wall", rds_tool_src, "-o", RDS_TOOL, "-L" + LIB_DIR, "-ldropest_facade", "-ldropest_amd",
         "-Wl,-rpath,$ORIGIN/../../dropest_amd/lib"],
        ["g++", "-O2", "-std=c++17", "-Wall", sharded_bam_src, "-o", SHARDED_BAM_TOOL, "-L" + LIB_DIR, "-ldropest_facade", "-ldropest_amd",
         "-Wl,-rpath,$ORIGIN/../../dropest_amd/lib"],
        ["g++", "-O2", "-std=c++17", "-Wall", validation_src, "-o", VALIDATION_TOOL, "-L" + LIB_DIR, "-ldropest_facade", "-ldropest_amd",
         "-Wl,-rpath,$ORIGIN/../../dropest_amd/lib"],
        ["g++", "-O2", "-std=c++17", "-Wall", validation_sharded_src, "-o", VALIDATION_SHARDED_TOOL, "-L" + LIB_DIR, "-ldropest_facade", "-ldropest_amd",
         "-Wl,-rpath,$ORIGIN/../../dropest_amd/lib"],
        ["g++", "-O2", "-std=c++17", "-Wall", tagged_src, "-o", TAGGED_TOOL, "-L" + LIB_DIR, "-ldropest_facade", "-ldropest_amd",
         "-Wl,-rpath,$ORIGIN/../../dropest_amd/lib"],
        ["g++", "-O2", "-std=c++17", "-Wall", umi_targets_src, "-o", UMI_TARGETS_TOOL, "-L" + LIB_DIR, "-ldropest_facade", "-ldropest_amd",
         "-Wl,-rpath,$ORIGIN/../../dropest_amd/lib"],
        ["g++", "-O2", "-std=c++17", "-Wall", filtered_src, "-o", FILTERED_TOOL, "-L" + LIB_DIR, "-ldropest_facade", "-ldropest_amd",
         "-Wl,-rpath,$ORIGIN/../../dropest_amd/lib"],
        ["g++", "-O2", "-std=c++17", "-Wall", filtered_sharded_src, "-o", FILTERED_SHARDED_TOOL, "-L" + LIB_DIR, "-ldropest_facade", "-ldropest_amd",
         "-Wl,-rpath,$ORIGIN/../../dropest_amd/lib"],
        ["g++", "-O2", "-std=c++17", "-Wall", corrections_src, "-o", CORRECTIONS_TOOL, "-L" + LIB_DIR, "-ldropest_facade", "-ldropest_amd",
         "-Wl,-rpath,$ORIGIN/../../dropest_amd/lib"],
        ["g++", "-O2", "-std=c++17", "-Wall", sources_src, "-o", SOURCES_TOOL, "-L" + LIB_DIR, "-ldropest_facade", "-ldropest_amd",
         "-Wl,-rpath,$ORIGIN/../../dropest_amd/lib"],
        ["g++", "-O2", "-std=c++17", "-Wall", sources_output_src, "-o", SOURCES_OUTPUT_TOOL, "-L" + LIB_DIR, "-ldropest_facade", "-ldropest_amd",
         "-Wl,-rpath,$ORIGIN/../../dropest_amd/lib"],
    ]
    for cmd in cmds:
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
    return FACADE_LIB, FACADE_TEST


if __name__ == "__main__":
    print(build(force=True, verbose=True))
    print(build_facade(force=True, verbose=True))
