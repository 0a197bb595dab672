"""The owners of device and page-locked buffers (gr_baz_amd/csrc/device_buffer.hip.h), without a GPU: a stand-alone C++
program (tests/c_abi/device_buffer_check.cc, its own main, nothing but the header) over a counting malloc / free policy,
built with AddressSanitizer and UndefinedBehaviorSanitizer and run as an ordinary program -- a leak, a double free or a
use after free ends it with a report, a failed check with the line."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gr_baz_amd", "csrc")
SOURCE = os.path.join(ROOT, "tests", "c_abi", "device_buffer_check.cc")


def _compilers():
    """g++ and the ROCm clang++, whichever are there (at least one: the libraries themselves need a C++ compiler)"""
    found = {}
    for c in (shutil.which("g++"), shutil.which("clang++"), "/opt/rocm/llvm/bin/clang++"):
        if c and os.path.exists(c):
            found.setdefault(os.path.realpath(c), c)      # (one name per program: it is run under the name that makes it a C++ driver)
    return sorted(found.values())


@pytest.mark.parametrize("cxx", _compilers(), ids=lambda c: os.path.basename(c).replace("-", "_"))
def test_owners_under_sanitizers(cxx, tmp_path):
    exe = str(tmp_path / "device_buffer_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", CSRC, "-o", exe, SOURCE]
    if "clang" not in os.path.basename(cxx):
        cmd[1:1] = ["-static-libasan", "-static-libubsan"]      # (clang links the runtimes into the program by default)
    build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, "%s\n%s" % (" ".join(cmd), build.stderr)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "checks hold" in run.stdout


def test_header_has_no_hip_include():
    """The header is plain C++ where no HIP runtime came first: that is what lets the program above include it alone."""
    text = open(os.path.join(CSRC, "device_buffer.hip.h")).read()
    assert "#include <hip" not in text and '#include "hip' not in text
