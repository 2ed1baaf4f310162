"""The oracle against the reference's own kernels executed on the host (oracle/reference.py, oracle/ref_host/): bit
for bit in pos, vel, rho, prs and force after every step, on the goldens, every grid of tests/grid_states.py, the
clicks, the cut-offs, other h, the nasty states and the reference's two initialisers.  The reference's lists are
built by a race; each step its build kernel's threads run in the order that makes every list read in the oracle's
canonical order, and from there the reference's text decides every operation (tests/reference_pin_cases.py).

Needs the reference build that build() makes where the reference's sources are present.  Absent sources: skipped.
Sources present and no library: a failure, not a skip."""
import os
import subprocess
import sys

import numpy as np
import pytest

import __graft_entry__ as entry
import grid_states as G
import reference_pin_cases as P
from helpers import dense_block
from oracle import oracle as O
from oracle import reference as R
from test_gpu_linked import REL, rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_OUT = os.path.join(ROOT, "oracle", "_ref")
REF_SRC = entry._reference_src()            # build()'s own lookup

needs_sources = pytest.mark.skipif(REF_SRC is None, reason="the reference's sources are not on this machine")


@pytest.fixture(scope="module")
def ref_build():
    assert R.available(), "the reference's sources are present but build() left no oracle/_ref/libsph_reference.so"
    return R.lib()


@needs_sources
def test_reference_simulator_compiled_against_its_own_headers(ref_build):
    """simulator.h and times.h of the host object are the reference's, cuda_runtime.h is oracle/ref_host's, and
    nothing of include/ was on its path (make's .d file, as tests/test_dropin.py reads the front end's)."""
    with open(os.path.join(REF_OUT, "simulator_host.d")) as f:
        deps = f.read().replace("\\\n", " ").split(":", 1)[1].split()
    src = os.path.abspath(REF_SRC)
    for h in ("simulator.h", "times.h"):
        assert [d for d in deps if os.path.basename(d) == h] == [os.path.join(src, h)]
    for h in ("cuda_runtime.h", "cuda_gl_interop.h"):
        assert [d for d in deps if os.path.basename(d) == h] == ["ref_host/" + h]
    assert not [d for d in deps if d.startswith("../include") or "/rocm" in d]


@needs_sources
@pytest.mark.parametrize("name", [n for n in P.BUILDERS])
def test_oracle_equals_the_reference_kernels(name, ref_build):
    """STEP_GRIDS, the h cases, the cut-offs and the nasty states: four steps.  D1: one (its second step would start
    outside the grid).  The click grids: a click at CLICK and at both EDGE_CLICKS on steps 1, 2, 3, then a plain step."""
    c = P.case(name)
    assert c.steps == (1 if name == "D1" else 4)
    want = P.oracle_run(c)
    if name.startswith("click"):
        plain = P.oracle_run(P.Case(c.name, c.pos, c.vel, c.h, c.cells, 1))
        G.assert_click_applied(plain[0]["vel"], want[0]["vel"], G.click_state(name.split()[1])[2])
    if name == "cut-offs":
        assert (want[0]["rho"] > G.REST_DENSITY).any(), "the pressure term must run"
    P.assert_same_steps(P.reference_run(c, want), want, name)


def _golden(name, ref, ora, steps):
    P.run_golden(ref, ora, np.load(os.path.join(ROOT, "tests", "golden", name + ".npz")), steps, name)


@needs_sources
def test_golden_grid2048_from_the_reference_setup(ref_build):
    """The reference's own setup() -i grid, 100 steps: every step equals the oracle's, every array grid2048.npz
    stores equals what the reference's code computes; and sph_initial_positions is that setup()."""
    import ctypes as C
    import cudafluidsimulator_amd as sph
    ref, ora = R.ReferenceSim(2048, False), O.OracleSim(2048, False)
    ref.setup()
    ora.setup()
    start = ref.download()
    assert P.differing(start["pos"], O.init_positions(O.make_settings(2048, False))) == 0
    lib_pos = np.zeros((2048, 3), np.float32)
    s = sph.default_settings(2048, False)
    assert sph.load_library().sph_initial_positions(C.byref(s), lib_pos.ctypes.data_as(C.POINTER(C.c_float))) == 0
    assert P.differing(start["pos"], lib_pos) == 0
    assert not start["vel"].any() and not start["rho"].any() and not start["prs"].any()
    _golden("grid2048", ref, ora, 100)


@needs_sources
def test_golden_dense4096(ref_build):
    pos = dense_block(16)
    ref, ora = R.ReferenceSim(len(pos), False), O.OracleSim(len(pos), False)
    ref.upload(pos)
    ora.upload(pos)
    _golden("dense4096", ref, ora, 20)


@needs_sources
@pytest.mark.parametrize("what", ["random-setup", "random4096"])
def test_reference_random_setup_in_a_fresh_process(what, ref_build):
    """setup() -i random consumes the process's rand(): a child process each.  random-setup: its positions equal
    oracle.init_positions and sph_initial_positions.  random4096: the golden from that setup(), 100 steps."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "reference_pin_cases.py"), what],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and f"child ok: {what}" in r.stdout, r.stdout[-1000:] + r.stderr[-3000:]


@needs_sources
def test_the_schedule_decides_the_bits_and_only_the_rounding(ref_build):
    """One step of the dense block with the build kernel's threads ascending instead of in the canonical schedule:
    rho is NOT bit-identical (the hook is real), and rho and pos agree within the 1e-5 relative bound that
    tests/test_gpu_linked.py uses for the race-ordered sweep, for exactly this reason (DESIGN.md section 2 has the
    measured spreads of one and twenty steps)."""
    pos = dense_block(16)
    n = len(pos)
    out = {}
    for name, order in (("canonical", np.arange(n)), ("ascending", np.arange(n)[::-1])):
        ref = R.ReferenceSim(n, False)
        ref.upload(pos)
        ref.step(order=order)        # lists read in `order`: the threads ran in its reverse
        out[name] = ref.download()
        ref.close()
    ref = R.ReferenceSim(n, False)
    ref.upload(pos)
    ref.step()                       # no schedule: descending threads, the canonical order after an upload
    assert P.differing(ref.download()["rho"], out["canonical"]["rho"]) == 0
    ref.close()
    a, c = out["ascending"], out["canonical"]
    words = P.differing(a["rho"], c["rho"])
    spread_rho = float(np.abs(a["rho"] - c["rho"]).max() / c["rho"].max())
    print(f"ascending vs canonical: {words} of {n} rho words differ, {spread_rho:.3g} of the largest rho; "
          f"pos: {P.differing(a['pos'], c['pos'])} words, rel {rel_err(a['pos'], c['pos'], 1e-3):.3g}")
    assert words > 0, "the schedule changed nothing: the hook is not real"
    assert rel_err(a["rho"], c["rho"], 1e-30) <= REL
    assert rel_err(a["pos"], c["pos"], 1e-3) <= REL


@needs_sources
def test_pin_file_is_what_the_reference_build_produces(ref_build):
    with open(P.PIN_JSON) as f:
        assert f.read() == P.dump(P.reference_digests()), "regenerate: python tests/golden/make_golden.py --reference"


@pytest.mark.parametrize("name", P.JSON_CASES)
def test_oracle_reproduces_the_pinned_digests(name):
    """Needs no reference: the oracle as THIS machine's compiler built it against the digests of the reference's
    kernels.  Inputs first: a numpy that drew other states is reported as that."""
    pin = P.load_pins()[name]
    c = P.case(name)
    assert (P.sha(c.pos), P.sha(c.vel)) == (pin["input"]["pos"], pin["input"]["vel"]), f"{name}: inputs differ"
    got = P.digests(c, P.oracle_run(c))
    assert {k: got[k] for k in ("n", "h", "cells", "clicks")} == {k: pin[k] for k in ("n", "h", "cells", "clicks")}
    for k, want in pin["steps"].items():
        for key in P.DIGESTED:
            assert got["steps"][k][key] == want[key], f"{name}, step {k}: the oracle's {key} is not the reference's"
    assert set(got["steps"]) == set(pin["steps"])


@needs_sources
def test_reference_host_build_is_clean_under_asan_and_ubsan():
    """A program of its own (oracle/ref_host/reference_selftest.cpp + the driver + the reference's simulator, all
    instrumented): two small in-grid cases, one with a schedule and a click.  Leak checking is off: the reference's
    setup() never frees its staging array."""
    b = subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), "ref-sanitize", "REF_SRC=" + os.path.abspath(REF_SRC)],
                       capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stdout[-2000:] + b.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(REF_OUT, "san", "reference_selftest")], capture_output=True, text=True,
                       timeout=300, env=env)
    assert r.returncode == 0 and "reference self-test: done" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]
