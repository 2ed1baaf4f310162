"""The strict list, lds and direct sweeps against tests/golden/reference_pin.json: the sha256 of pos, vel, rho and prs
by particle id after every step, as the REFERENCE's own kernels produce them on the host under the canonical build
schedule (tests/reference_pin_cases.py; written by tests/golden/make_golden.py --reference where the reference is
present).  Cut-offs, D2, D7, D102, D257, the (0.3, 33) click grid with its three clicks, h = 0.01 and h = 1.0; the
largest case has 3001 rows.  Reads the JSON only.  A mismatch names the array and counts the words that differ from
the live oracle -- none there means the oracle of this machine left the reference too."""
import functools

import pytest

import cudafluidsimulator_amd as sph
import reference_pin_cases as P

pytestmark = pytest.mark.gpu
SWEEPS = ["list", "lds", "direct"]


@functools.lru_cache(maxsize=None)
def pinned(name):
    """the case, its JSON entry, and (lazily, once for the three sweeps) the live oracle's run"""
    return P.case(name), P.load_pins()[name]


@functools.lru_cache(maxsize=None)
def live_oracle(name):
    return P.oracle_run(pinned(name)[0])


@pytest.mark.parametrize("sweep", SWEEPS)
@pytest.mark.parametrize("name", P.JSON_CASES)
def test_strict_sweeps_reproduce_the_reference_digests(name, sweep):
    c, pin = pinned(name)
    assert (P.sha(c.pos), P.sha(c.vel)) == (pin["input"]["pos"], pin["input"]["vel"]), f"{name}: inputs differ"
    assert (len(c.pos), c.h, c.cells, c.steps) == (pin["n"], pin["h"], pin["cells"], len(pin["steps"]))
    assert {str(k): list(v) for k, v in c.clicks.items()} == pin["clicks"]
    sim = sph.Simulator(c.settings(factory=sph.default_settings), sweep=sweep)
    sim.upload_state(c.pos, c.vel)
    for k in range(1, c.steps + 1):
        sim.simulate()
        if k in c.clicks:
            sim.moveParticles(c.clicks[k])           # sph_apply_click
        got = sim.download_state()
        for key in P.DIGESTED:
            if P.sha(got[key]) != pin["steps"][str(k)][key]:
                want = live_oracle(name)[k - 1][key]
                pytest.fail(f"{name} {sweep}, step {k}: {key} is not the reference's; {P.differing(got[key], want)} of "
                            f"{want.size} words differ from the live oracle")
    sim.close()
