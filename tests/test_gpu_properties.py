"""Full-size checks (BASELINE.json configs 2 and 3) through size-independent
properties, plus bounded oracle comparisons at those sizes."""
import numpy as np
import pytest

import cudafluidsimulator_amd as sph
from cudafluidsimulator_amd import _lib
from helpers import assert_bit_equal
from oracle import oracle as O

pytestmark = pytest.mark.gpu


def run(n, steps, sweep="list", flags=0):
    sim = sph.Simulator(sph.default_settings(n, True), sweep=sweep, flags=flags)
    sim.setup()
    for _ in range(steps):
        sim.simulate()
    return sim


def test_config2_262144_all_sweeps_equal_and_oracle():
    a = run(262144, 12, "list", _lib.SPH_FLAG_COUNT_PAIRS)
    b = run(262144, 12, "direct")
    c = run(262144, 12, "lds")
    sa, sb, sc = a.download_state(), b.download_state(), c.download_state()
    for k in sa:
        assert_bit_equal(sa[k], sb[k], k)
        assert_bit_equal(sa[k], sc[k], k + " (lds)")
    c.close()
    ref = O.OracleSim(262144, True)
    ref.setup()
    want_tests = 0
    for _ in range(12):
        ref.step()
        want_tests += ref.last_pair_tests()
    assert_bit_equal(sa["pos"], ref.download()["pos"], "oracle")
    kt = a.kernel_times()
    assert kt.steps == 12 and kt.pair_tests == want_tests   # exact: the oracle's count, step by step
    assert kt.pair_tests > 12 * 3.5e6
    a.close(); b.close()


def test_config3_4194304_invariants_and_determinism():
    n, steps = 4194304, 4
    a = run(n, steps, flags=_lib.SPH_FLAG_COUNT_PAIRS)
    g = a.download_grid()
    assert np.array_equal(np.sort(g["ids"]), np.arange(n, dtype=np.uint32))   # permutation
    assert (np.diff(g["keys"].astype(np.int64)) >= 0).all()                    # sortedness
    cnt = g["cells"][:, 1] - g["cells"][:, 0]
    assert cnt.sum() == n and (cnt >= 0).all()                                 # cells partition
    st = a.download_state()
    h, hi = np.float32(0.1), np.float32(10.0) - np.float32(0.1)
    assert (st["pos"] >= h).all() and (st["pos"] <= hi).all()
    assert np.isfinite(st["vel"]).all() and (st["rho"] >= 31.3).all()
    assert_bit_equal(np.array(a.getPosition()), st["pos"], "getPosition order")
    kt = a.kernel_times()
    assert 8.5e8 * steps < kt.pair_tests < 9.6e8 * steps  # 9.09e8/sweep
    b = run(n, steps)                                      # run-to-run bit reproducible
    assert_bit_equal(b.download_state()["pos"], st["pos"], "determinism")
    b.close()
    # bounded oracle comparison at full size: 2 steps
    ref = O.OracleSim(n, True)
    ref.setup()
    want_tests = 0
    for _ in range(2):
        ref.step()
        want_tests += ref.last_pair_tests()
    c = run(n, 2)
    assert_bit_equal(c.download_state()["pos"], ref.download()["pos"], "oracle 2 steps @4M")
    d = run(n, 2, flags=_lib.SPH_FLAG_COUNT_PAIRS)          # (a handle of its own: the parity run above keeps flags = 0)
    assert d.kernel_times().pair_tests == want_tests        # exact: the oracle's count of the first two sweeps
    d.close()
    assert 8.5e8 * 2 < want_tests < 9.6e8 * 2
    a.close(); c.close()


def _invariants(sim, n):
    g = sim.download_grid()
    assert np.array_equal(np.sort(g["ids"]), np.arange(n, dtype=np.uint32))
    assert (np.diff(g["keys"].astype(np.int64)) >= 0).all()
    cnt = g["cells"][:, 1] - g["cells"][:, 0]
    assert cnt.sum() == n and (cnt >= 0).all()
    st = sim.download_state()
    h, hi = np.float32(0.1), np.float32(10.0) - np.float32(0.1)
    assert (st["pos"] >= h).all() and (st["pos"] <= hi).all()
    assert np.isfinite(st["vel"]).all() and np.isfinite(st["rho"]).all()
    return st, cnt


def test_config4_16777216_random_variants_agree():
    """BASELINE.json configs[3] size on ONE GPU (the 4-GPU slab run of it cannot be
    launched here): invariants, and the default hit-mask sweeps agree bit for bit
    with the LDS/FIFO sweeps -- two independent kernel families, no oracle needed."""
    n, steps = 16777216, 2
    a = run(n, steps, "list")
    st, cnt = _invariants(a, n)
    assert cnt.max() < 200
    b = run(n, steps, "lds")
    assert_bit_equal(b.download_state()["pos"], st["pos"], "list vs lds @16.7M")
    a.close(); b.close()


def test_config5_67108864_dense_lattice_extension():
    """BASELINE.json configs[4]: -n 67108864 -i grid is OUTSIDE the reference's
    domain (its lattice holds 109^3 points, simulator.cu:439-452); the labelled
    dense-lattice extension runs, pressure is active from step 1 (rho > 1000), and
    the mask pool either suffices or falls back per wave -- same answer as LDS."""
    n = 67108864
    s = sph.default_settings(n, False)
    a = sph.Simulator(s, sweep="list")
    a.setup()
    a.simulate()
    st, cnt = _invariants(a, n)
    assert st["rho"].max() > 1000 and (st["prs"] > 0).sum() > n // 4
    pos_a = st["pos"].copy()
    del st
    a.close()
    b = sph.Simulator(s, sweep="lds")
    b.setup()
    b.simulate()
    assert_bit_equal(b.download_state()["pos"], pos_a, "list vs lds @67M dense lattice")
    b.close()


def test_config5_67108864_eight_slabs_equal_single_domain():
    """BASELINE.json configs[4] at FULL size through the C++ multi-GPU driver: eight
    z-slabs (the loopback transport puts them on this one GPU) of the 67,108,864-particle
    dense lattice -- 71 particles per cell, pressure on from step 1, halo layers of ~0.68 M
    particles -- against the single domain, one step, bit for bit."""
    from cudafluidsimulator_amd import mgpu as M
    n = 67108864
    s = sph.default_settings(n, False)
    mg = M.MultiGpuSimulator(s, world=8, transport="loopback")
    mg.setup()
    mg.simulate()
    got = mg.download_state()
    st = mg.stats()
    mg.close()
    assert got["written"] == n and st.host_syncs == 1
    a = sph.Simulator(s, sweep="list")
    a.setup()
    a.simulate()
    want = a.download_state()
    a.close()
    assert (want["rho"] > 1000).sum() > n // 4
    assert_bit_equal(got["pos"], want["pos"], "67M dense lattice, 8 slabs vs single domain: pos")
    assert_bit_equal(got["rho"], want["rho"], "67M dense lattice, 8 slabs vs single domain: rho")


def test_headline_config_beyond_the_goldens_list_equals_lds():
    """Past the 100 steps the goldens cover the fluid keeps piling up on the floor (hundreds of
    particles per cell, rho several times the rest density): runs far longer than the LDS slice,
    the largest hit-stream reservations.  Two kernel families must still agree bit for bit."""
    n, steps = 4194304, 150
    a = run(n, steps, "list")
    sa = a.download_state()
    g = a.download_grid()
    assert (g["cells"][:, 1] - g["cells"][:, 0]).max() > 150
    a.close()
    b = run(n, steps, "lds")
    sb = b.download_state()
    b.close()
    for k in ("pos", "vel", "rho"):
        assert_bit_equal(sa[k], sb[k], k + " @ step 150")


def _sha(a):
    import hashlib
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _golden(name):
    import json
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name)
    if not os.path.exists(path):
        pytest.skip(name + " not generated (tests/golden/make_golden.py)")
    return json.load(open(path))


def test_config4_16777216_matches_the_oracles_checksums():
    """BASELINE configs[3] at full size against the ORACLE (sha256 of its arrays after steps 1
    and 2, tests/golden/make_golden.py --config4): 32.8 particles per cell, 21 k particles
    with pressure on in the very first step."""
    g = _golden("random16777216_sha256.json")
    n = g["n"]
    sim = sph.Simulator(sph.default_settings(n, True))
    sim.setup()
    done = 0
    for k in sorted(int(x) for x in g["steps"]):
        for _ in range(k - done):
            sim.simulate()
        done = k
        st = sim.download_state()
        assert _sha(st["pos"]) == g["steps"][str(k)]["pos_sha256"], f"pos @ step {k}"
        assert _sha(st["rho"]) == g["steps"][str(k)]["rho_sha256"], f"rho @ step {k}"
    sim.close()


def test_config5_67108864_matches_the_oracles_checksum():
    """BASELINE configs[4] (the dense-lattice extension) at full size against the ORACLE: sha256
    of its position and density arrays after the first step (71 particles per cell, 1.3e11 pair
    tests per sweep, pressure on everywhere; tests/golden/make_golden.py --config5)."""
    g = _golden("grid67108864_sha256.json")
    n = g["n"]
    sim = sph.Simulator(sph.default_settings(n, False))
    sim.setup()
    sim.simulate()
    st = sim.download_state()
    assert _sha(st["pos"]) == g["steps"]["1"]["pos_sha256"], "pos @ step 1"
    assert _sha(st["rho"]) == g["steps"]["1"]["rho_sha256"], "rho @ step 1"
    sim.close()


def test_headline_config_in_eight_slabs_matches_the_oracles_checksums():
    """The multi-GPU driver at full size: -n 4194304 -i random cut into 8 z-slabs (the RCCL path's stream
    layout with event-ordered copies as messages, all slabs on this GPU) against the ORACLE's sha256 of
    the positions at every golden step through step 100 -- the floor pile, pressure on, particles
    migrating between slabs, the dealt force sweep on interior and boundary ranges."""
    from cudafluidsimulator_amd import mgpu as M
    g = _golden("random4194304_sha256.json")
    mg = M.MultiGpuSimulator(sph.default_settings(g["n"], True), world=8, transport="streams")
    mg.setup()
    done = 0
    for k in sorted(int(x) for x in g["steps"]):
        for _ in range(k - done):
            mg.simulate()
        done = k
        assert _sha(mg.download_state()["pos"]) == g["steps"][str(k)]["pos_sha256"], f"pos @ step {k}"
    assert _sha(np.array(mg.getPosition())) == g["steps"][str(done)]["pos_sha256"], "getPosition()"
    mg.close()


def test_morton_order_at_full_size_matches_the_morton_keyed_oracle():
    """SPH_KEY_MORTON (BASELINE config 3's ordering) at n = 4,194,304 against the oracle run with the
    Morton key function: sha256 after steps 1 and 3 of a state that migrates along all three axes
    (tests/golden/make_golden.py --morton; the all-at-rest start does not tell the two key functions
    apart).  The same input under the flattened key reproduces the flattened oracle's digests, and
    those differ from the Morton ones at step 3: the key function changes the summation order."""
    import importlib.util
    import os
    g = _golden("random4194304_morton_sha256.json")
    spec = importlib.util.spec_from_file_location(
        "make_golden", os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    n = g["n"]
    pos, vel = mg.morton_state(n, g["seed"])
    for ko, want in (("morton", g["steps"]), ("flattened", g["flattened_steps"])):
        sim = sph.Simulator(sph.default_settings(n, True), sweep="direct" if ko == "morton" else "list", key_order=ko)
        sim.upload_state(pos, vel)
        done = 0
        for k in sorted(int(x) for x in want):
            for _ in range(k - done):
                sim.simulate()
            done = k
            st = sim.download_state()
            assert _sha(st["pos"]) == want[str(k)]["pos_sha256"], f"{ko}: pos @ step {k}"
            assert _sha(st["rho"]) == want[str(k)]["rho_sha256"], f"{ko}: rho @ step {k}"
        sim.close()
    assert g["steps"]["3"]["pos_sha256"] != g["flattened_steps"]["3"]["pos_sha256"]
