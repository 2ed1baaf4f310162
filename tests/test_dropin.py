"""Drop-in checks against the reference's own front end.  The times table is compared with
the bytes the reference's times.h prints for the same program (recorded once under
tests/golden/reference_times_table.txt).  The reference's unmodified main.cpp and
display.cpp are compiled against OUR headers by build() (oracle/Makefile, target ref) into
oracle/_ref/ when the reference's sources are present; nothing from the reference is
committed, and these tests read only what build() left there."""
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_OUT = os.path.join(ROOT, "oracle", "_ref")
GOLD_TABLE = os.path.join(ROOT, "tests", "golden", "reference_times_table.txt")

needs_ref = pytest.mark.skipif(not os.path.exists(os.path.join(REF_OUT, "main.o")),
                               reason="the reference's front end was not built (oracle/_ref: reference absent)")

PROG = r"""
#include "times.h"
int main() { Times t; t.buildGrid = 0.123456; t.sphUpdate = 1.5; t.memcpy = 0.0421; t.iters = 100;
  displayTimes(&t); Times z; displayTimes(&z); return 0; }
"""


def _table(include_dir):
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.cpp")
        open(src, "w").write(PROG)
        exe = os.path.join(d, "t")
        subprocess.check_call(["g++", "-std=c++17", "-I" + include_dir, src, "-o", exe])
        return subprocess.check_output([exe])


def test_times_table_is_byte_identical_to_reference():
    with open(GOLD_TABLE, "rb") as f:
        assert _table(os.path.join(ROOT, "include")) == f.read()


def test_times_table_known_bytes():
    out = _table(os.path.join(ROOT, "include")).decode().split("\n")
    assert out[0] == "Operation            Per frame       Total"
    assert out[2] == "Grid construction    0.00123        0.12346"
    assert out[3] == "SPH update           0.01500        1.50000"
    assert out[4] == "Data transfer        0.00042        0.04210"


def _deps(src):
    """Headers one object of the reference's front end was compiled against (make's .d file)."""
    with open(os.path.join(REF_OUT, src.replace(".cpp", ".d"))) as f:
        return f.read().replace("\\\n", " ").split(":", 1)[1].split()


@needs_ref
@pytest.mark.parametrize("src", ["main.cpp", "display.cpp"])
def test_reference_front_end_compiles_against_our_headers(src):
    """The reference's unmodified main.cpp / display.cpp compile with OUR simulator.h +
    times.h (the text is piped to g++ so its quoted includes resolve through -iquote, ours
    first), the types-only cuda_runtime.h and prototype-only GL stubs (oracle/ref_stubs)."""
    assert os.path.getsize(os.path.join(REF_OUT, src.replace(".cpp", ".o"))) > 0
    deps = _deps(src)
    for h in ("simulator.h", "times.h"):
        used = [d for d in deps if os.path.basename(d) == h]
        assert used == ["../include/" + h], used


@needs_ref
def test_reference_main_builds_and_links_against_library():
    """Link the reference's main.cpp (compiled against our headers by build()) with our
    simulator + headless stub + libsph_hip.so (+ libsph_mgpu.so, the SPH_GPUS=N path of the
    same Simulator class) and run its argument check -- the rest needs a GPU."""
    lib = os.path.join(ROOT, "cudafluidsimulator_amd", "libsph_hip.so")
    csrc = os.path.join(ROOT, "cudafluidsimulator_amd", "csrc")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "sph_refmain")
        subprocess.check_call(["g++", "-o", exe, os.path.join(REF_OUT, "main.o"), os.path.join(csrc, "simulator.o"),
                               os.path.join(csrc, "headless.o"),
                               os.path.join(os.path.dirname(lib), "libsph_mgpu.so"), lib,
                               "-Wl,-rpath," + os.path.dirname(lib)])
        out = subprocess.run([exe, "-i", "bogus"], capture_output=True, text=True)
        assert out.returncode == 1 and "Invalid argument for option -i" in out.stdout
