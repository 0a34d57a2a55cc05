"""Builds the stand-alone check programs of tests/native/ that link the host pipeline's four sources, plain or under a sanitizer.
The four sources are compiled once per set of flags for all the test files of a run (nothing is loaded into Python)."""
import atexit
import functools
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mitoflex_amd", "csrc")
NATIVE = os.path.join(ROOT, "tests", "native")
HOST_SRCS = ["mf_pipeline.cpp", "mf_host.cpp", "mf_inflate.cpp", "mf_pinflate.cpp"]
FLAG_SETS = [(), ("-fsanitize=address,undefined", "-fno-omit-frame-pointer"), ("-fsanitize=thread",)]
FLAG_IDS = ["plain", "asan_ubsan", "tsan"]


@functools.lru_cache(None)
def _dir():
    d = tempfile.mkdtemp(prefix="mf_native_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    return d


def _tag(flags):
    return "_".join(f.replace("=", "").replace(",", "").replace("-", "") for f in flags) or "plain"


def _compile(srcs, flags, tag):
    """every source to an object of its own, side by side"""
    jobs = []
    for s in srcs:
        o = os.path.join(_dir(), os.path.basename(s) + "." + tag + ".o")
        jobs.append((o, subprocess.Popen(["g++", "-O1", "-g", "-std=c++17", *flags, "-I", CSRC, "-c", s, "-o", o])))
    for o, p in jobs:
        assert p.wait() == 0, o
    return [o for o, _ in jobs]


@functools.lru_cache(None)
def host_objects(flags):
    return tuple(_compile([os.path.join(CSRC, s) for s in HOST_SRCS], flags, _tag(flags)))


@functools.lru_cache(None)
def build_check(names, flags=()):
    """names: sources of tests/native (the first names the program) -> path of the program, linked with the host sources"""
    exe = os.path.join(_dir(), names[0].replace(".cpp", "") + "_" + _tag(flags))
    objs = _compile([os.path.join(NATIVE, n) for n in names], flags, _tag(flags))
    subprocess.check_call(["g++", *flags, *objs, *host_objects(flags), "-lz", "-lpthread", "-o", exe])
    return exe


def clean(stderr):
    """no sanitizer report in what a check program wrote to stderr"""
    err = stderr.decode(errors="replace")
    assert "Sanitizer" not in err and "runtime error" not in err, err[:3000]
    return err
