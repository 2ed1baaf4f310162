"""`./sph -m free` as a user runs it (headless.cpp over the C++ `Simulator` of simulator.cpp):
every output of a frame at once against each output alone, file for file and line for line, on the three strict
sweeps and the four frame kinds; SPH_FREE_FRAME_EVERY with the two outputs that carry state from frame to frame
(tracers, tracks) against the Python binding doing what headless.cpp documents; the same command line over slabs
(SPH_GPUS with the loopback and the streams transport, with re-cuts): the queued click, the statistics a multi-GPU run
still writes and the outputs it refuses, each once; and SPH_SWEEP=linked, which refuses every walking output once and
goes on with the frames and the statistics."""
import hashlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

import cudafluidsimulator_amd as sph
from cudafluidsimulator_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPH = os.path.join(ROOT, "cudafluidsimulator_amd", "sph")
F = np.float32
N = 32768  # in [1, 9]^3 about 0.27 neighbours within h each: test_the_state_has_what_the_outputs_need holds that this is enough
FRAMES = 5
CLICK_FRAME = FRAMES // 2  # headless.cpp sets mouseClicked before frame frames / 2; simulate() applies it after that step
TRACERS = 100
TRACK_LINK = 0.75  # of h; bodies: 1, the table: 0.5 -- three labellings a frame, so a table of the wrong one shows
ISO = 1.0          # tests/test_gpu_surface.py


# what switches each of the twelve outputs on, and the files it writes beside the flat frames
OUTPUTS = {
    "shade": {"SPH_FREE_SHADE": "speed"},
    "slice": {"SPH_FREE_SLICE": "density"},
    "surface": {"SPH_FREE_SURFACE": str(ISO)},
    "tracers": {"SPH_FREE_TRACERS": str(TRACERS)},
    "particles": {"SPH_FREE_PARTICLES": "1"},
    "bodies": {"SPH_FREE_BODIES": "1"},
    "body_table": {"SPH_FREE_BODY_TABLE": "0.5"},
    "body_tracks": {"SPH_FREE_BODY_TRACKS": str(TRACK_LINK)},
    "neighbours": {"SPH_FREE_NEIGHBOURS": "1"},
    "pair_stats": {"SPH_FREE_PAIR_STATS": "16"},
    "stats": {"SPH_FREE_STATS": "1"},
    "flat": {},
}
EVERYTHING = {k: v for name, env in OUTPUTS.items() if name != "shade" for k, v in env.items()}  # (the frames: flat)
SAID = {"bodies ": "bodies", "tracks ": "body_tracks", "neighbours ": "neighbours", "pairs ": "pair_stats"}  # stderr lines
KEEP = re.compile(r"stats\.jsonl|tracers_\d+\.ply|body_tracks_\d+\.jsonl")  # the files a test reads again (the tracks: of section 2's runs)
SHADES = {"flat": {}, "speed": {"SPH_FREE_SHADE": "speed"}, "column": {"SPH_FREE_SHADE": "column"}, "liquid": {"SPH_FREE_SHADE": "liquid"}}


class Run:
    """One ./sph process: exit status, both streams, and of every file it wrote the size and the sha256 (`files`), of
    every .ply its header (`heads`).  Files no test reads again are removed once they are hashed."""

    def __init__(self, out, env_extra):
        env = {k: v for k, v in os.environ.items() if not k.startswith("SPH_")}
        env.update({"SPH_FREE_FRAMES": str(FRAMES), "SPH_PRINT_SHA256": "1", "SPH_FREE_FRAMES_DIR": str(out), **env_extra})
        r = subprocess.run([SPH, "-n", str(N), "-i", "random", "-m", "free"], capture_output=True, text=True, timeout=120, env=env)
        self.dir, self.returncode, self.stdout, self.stderr = out, r.returncode, r.stdout, r.stderr
        self.files, self.heads, self.lines = {}, {}, {}
        for name in sorted(os.listdir(out)):
            blob = open(out / name, "rb").read()
            self.files[name] = (len(blob), hashlib.sha256(blob).hexdigest())
            self.lines[name] = blob.count(b"\n")
            if name.endswith(".ply"):
                self.heads[name] = blob[:blob.index(b"end_header\n")].decode().split("\n")
            if not KEEP.fullmatch(name) or (len(blob) > (1 << 20) and "SPH_FREE_FRAME_EVERY" not in env_extra):
                os.remove(out / name)

    def said(self, prefix):
        return [l for l in self.stderr.splitlines() if l.startswith(prefix)]

    def sha(self):
        m = re.search(r"^positions_sha256 ([0-9a-f]{64})$", self.stdout, re.M)
        assert m, self.stdout + self.stderr
        return m.group(1)

    def read(self, name):
        return open(self.dir / name, "rb").read()


@pytest.fixture(scope="module")
def sph_run(tmp_path_factory):
    """sph_run(**env) -> Run, one process per distinct environment for the whole module, and one at a time"""
    made = {}

    def get(**env):
        key = tuple(sorted(env.items()))
        if key not in made:
            made[key] = Run(tmp_path_factory.mktemp("run"), env)
            assert made[key].returncode == 0, made[key].stderr
        return made[key]

    return get


def single(sph_run, name, **more):
    return sph_run(SPH_FREE_CLICK="1", **OUTPUTS[name], **more)


def combined(sph_run, shade="flat", **more):
    return sph_run(SPH_FREE_CLICK="1", **EVERYTHING, **SHADES[shade], **more)


def frames_of(names):
    return sorted({int(m.group(1)) for m in (re.search(r"_(\d{4})\.", x) for x in names) if m})


def assert_single_in_combined(one, all_, name):
    """every file of the run with one output is the combined run's file of that name; the lines on stderr are the same"""
    assert set(one.files) <= set(all_.files), (name, sorted(set(one.files) - set(all_.files)))
    differ = [x for x in one.files if one.files[x] != all_.files[x]]
    assert not differ, f"{name}: alone and with every other output these files differ: {differ}"
    for prefix, owner in SAID.items():
        assert one.said(prefix) == (all_.said(prefix) if owner == name else []), (name, prefix)
        assert len(all_.said(prefix)) == len(frames_of(all_.files)), (prefix, all_.stderr)
    assert one.sha() == all_.sha(), name


def oracle_sha():
    from oracle import oracle as O

    ref = O.OracleSim(N, True)
    ref.setup()
    for f in range(FRAMES):
        ref.step()
        if f == CLICK_FRAME:
            ref.click(400, 300)
    want = hashlib.sha256(np.ascontiguousarray(ref.download()["pos"]).tobytes()).hexdigest()
    ref.close()
    return want


# ---- 1. everything at once equals each output alone ----

def test_the_state_has_what_the_outputs_need(sph_run):
    """The floors the comparisons below rest on, from what the runs of one output each say themselves: pairs, bodies of
    more than one particle, bodies that go on from frame to frame, neighbours, a surface."""
    pairs =[l.split() for l in single(sph_run, "pair_stats").said("pairs ")]
    assert [int(p[1]) for p in pairs] == list(range(FRAMES)) and all(int(p[2]) >= 1000 for p in pairs), pairs
    bodies = [l.split() for l in single(sph_run, "bodies").said("bodies ")]
    assert len(bodies) == FRAMES and all(N - int(b[2]) >= 500 for b in bodies), bodies
    tracks = [l.split() for l in single(sph_run, "body_tracks").said("tracks ")]
    assert len(tracks) == FRAMES and int(tracks[-1][3]) > 0, tracks
    neighbours = [l.split() for l in single(sph_run, "neighbours").said("neighbours ")]
    assert len(neighbours) == FRAMES and int(neighbours[-1][2]) > 0, neighbours
    head = single(sph_run, "surface").heads["surface_%04d.ply" % (FRAMES - 1)]
    faces = [l for l in head if l.startswith("element face ")]
    assert len(faces) == 1 and int(faces[0].split()[-1]) > 0, head


@pytest.mark.parametrize("name", list(OUTPUTS))
def test_an_output_alone_writes_what_it_writes_among_all(sph_run, name):
    one = single(sph_run, name)
    assert_single_in_combined(one, combined(sph_run, "speed" if name == "shade" else "flat"), name)
    assert frames_of(one.files) == list(range(FRAMES)) and ("frame_%04d.ppm" % (FRAMES - 1)) in one.files


def test_all_outputs_at_once_write_the_union_and_end_on_the_oracles_positions(sph_run):
    all_ = combined(sph_run)
    ones = {name: single(sph_run, name) for name in OUTPUTS}
    assert set(all_.files) == set().union(*(o.files for o in ones.values()))
    assert len(all_.files) == 10 * FRAMES + 1, sorted(all_.files)  # the frames and nine more kinds of numbered files; stats.jsonl
    want = oracle_sha()
    assert all_.sha() == want
    assert {name: o.sha() for name, o in ones.items()} == {name: want for name in ones}
    assert "failed (" not in all_.stderr and not [l for l in all_.stderr.splitlines() if "multi-GPU" in l or "SPH_SWEEP_LINKED" in l]


def test_three_labellings_a_frame_keep_their_own_tables(sph_run):
    """A frame labels at h for the body files, at 0.5 h for the table and at 0.75 h for the tracks: a shorter link leaves
    more bodies, and each file has the rows of its own labelling (with 1,000 pairs spread over (0, h] strictly more)."""
    all_ = combined(sph_run)
    bodies = [int(l.split()[2]) for l in all_.said("bodies ")]
    tracked = [int(l.split()[2]) for l in all_.said("tracks ")]
    table = [all_.lines["body_table_%04d.jsonl" % f] for f in range(FRAMES)]
    print("bodies at h", bodies, "at 0.75 h", tracked, "rows of the table at 0.5 h", table)
    assert len(bodies) == len(tracked) == FRAMES
    assert all(a < b < c <= N for a, b, c in zip(bodies, tracked, table)), (bodies, tracked, table)


@pytest.mark.parametrize("sweep", ["lds", "direct"])
def test_every_strict_sweep_writes_the_same_files(sph_run, sweep):
    """all outputs are defined to the bit and all strict sweeps give the oracle's density"""
    base, other = combined(sph_run), combined(sph_run, SPH_SWEEP=sweep)
    assert other.files == base.files, [x for x in base.files if other.files.get(x) != base.files[x]]
    assert [other.said(p) for p in SAID] == [base.said(p) for p in SAID]
    assert other.sha() == base.sha()


@pytest.mark.parametrize("shade", list(SHADES))
def test_the_frame_kind_changes_the_frames_alone(sph_run, shade):
    base, all_ = combined(sph_run), combined(sph_run, shade)
    alone = sph_run(SPH_FREE_CLICK="1", **SHADES[shade])
    frames = ["frame_%04d.ppm" % f for f in range(FRAMES)]
    assert sorted(alone.files) == frames
    assert {x: all_.files[x] for x in frames} == alone.files
    rest = lambda r: {x: v for x, v in r.files.items() if x not in frames}
    assert rest(all_) == rest(base) and len(rest(base)) == 9 * FRAMES + 1
    assert shade == "flat" or all_.files[frames[-1]] != base.files[frames[-1]]


# ---- 2. SPH_FREE_FRAME_EVERY ----

WRITTEN = [0, 2, 4]


@pytest.mark.parametrize("name", list(OUTPUTS))
def test_frame_every_keeps_every_second_frame_of_each_output(sph_run, name):
    all_ = combined(sph_run, "speed" if name == "shade" else "flat", SPH_FREE_FRAME_EVERY="2")
    assert frames_of(all_.files) == WRITTEN and len(all_.files) == 10 * len(WRITTEN) + 1, sorted(all_.files)
    assert [json.loads(l)["frame"] for l in all_.read("stats.jsonl").splitlines()] == WRITTEN
    one = single(sph_run, name, SPH_FREE_FRAME_EVERY="2")
    assert frames_of(one.files) == WRITTEN
    assert_single_in_combined(one, all_, name)


def stepped(sim, f):
    """frame f of headless.cpp's loop on the Python binding"""
    if f == CLICK_FRAME:
        sim.mouseClicked, sim.clickCoords = True, (400, 300)
    sim.simulate()


def test_tracers_move_on_the_frames_that_are_not_written(sph_run):
    """Tracers are advected after every frame and written beside the kept ones."""
    all_ = combined(sph_run, SPH_FREE_FRAME_EVERY="2")
    sim = sph.Simulator(sph.default_settings(N, True))
    sim.setup()
    sim.set_tracers(np.array(sim.getPosition(), copy=True)[[k * N // TRACERS for k in range(TRACERS)]])
    moved = 0
    for f in range(FRAMES):
        stepped(sim, f)
        sim.advect_tracers(sim.settings.timestep)
        if f not in WRITTEN:
            continue
        t = sim.tracers()
        want = np.concatenate([t["pos"], t["vel"], t["den"][:, None]], axis=1).astype(F)
        blob = all_.read("tracers_%04d.ply" % f)
        assert all_.heads["tracers_%04d.ply" % f][2:] == ["element vertex %d" % TRACERS] + ["property float " + k for k in ("x", "y", "z", "vx", "vy", "vz", "density")] + [""]
        got = np.frombuffer(blob[blob.index(b"end_header\n") + 11:], "<f4").reshape(TRACERS, 7)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f
        moved += int((t["den"] > 0).sum())
    sim.close()
    assert moved > 0  # some tracers sit in fluid: velocities and densities that are not all zero


def test_tracks_refer_to_the_previous_written_frame(sph_run):
    """The reference of a frame's tracks is the labelling of the frame written before it, not of the frame before it."""
    all_ = combined(sph_run, SPH_FREE_FRAME_EVERY="2")
    said = [l.split() for l in all_.said("tracks ")]
    sim = sph.Simulator(sph.default_settings(N, True))
    sim.setup()
    TRACK_CONTINUES, MAIN_PARENT, MAIN_CHILD = _lib.SPH_TRACK_CONTINUES, _lib.SPH_EDGE_MAIN_PARENT, _lib.SPH_EDGE_MAIN_CHILD
    before = None
    for f in range(FRAMES):
        stepped(sim, f)
        if f not in WRITTEN:
            continue
        got = sim.track_bodies(TRACK_LINK * float(sim.settings.h))
        s, t, p, e = got["summary"], got["tracks"], got["previous"], got["edges"]
        lines = [json.loads(l) for l in all_.read("body_tracks_%04d.jsonl" % f).splitlines()]
        assert lines[0] == dict(frame=f, **s)
        assert lines[0]["previous_bodies"] == (0 if before is None else before), f
        assert len(lines) == 1 + len(t) + len(e) and len(t) > 1 and (f == 0 or len(e) >= len(t))
        table = got["table"]
        for b, line in enumerate(lines[1:1 + len(t)]):
            parent = int(p["label"][t["main_parent"][b]]) if t["parents"][b] else None
            assert line == dict(label=int(table[b, 0]), count=int(table[b, 1]), track=int(t["track"][b]), parents=int(t["parents"][b]),
                                main_parent=parent, main_overlap=int(t["main_overlap"][b]), continues=bool(t["flags"][b] & TRACK_CONTINUES)), (f, b)
        for k, line in enumerate(lines[1 + len(t):]):
            assert line == dict(prev=int(p["label"][e["prev"][k]]), cur=int(table[e["cur"][k], 0]), count=int(e["count"][k]),
                                main_parent=bool(e["flags"][k] & MAIN_PARENT), main_child=bool(e["flags"][k] & MAIN_CHILD)), (f, k)
        assert said[WRITTEN.index(f)] == ["tracks"] + [str(x) for x in (f, s["bodies"], s["continued"], s["born"], s["ended"], s["merges"], s["splits"])]
        before = s["bodies"]
    sim.close()
    assert len(said) == len(WRITTEN)


# ---- 3. -m free over slabs ----

SLABS = {
    "4-loopback": {"SPH_GPUS": "4", "SPH_TRANSPORT": "loopback"},
    "3-streams": {"SPH_GPUS": "3", "SPH_TRANSPORT": "streams"},
    "4-loopback-recut": {"SPH_GPUS": "4", "SPH_TRANSPORT": "loopback", "SPH_RECUT_EVERY": "2"},
}
NOT_RENDERED = "frames of a multi-GPU run (SPH_GPUS > 1) are not rendered"
REFUSED = "a multi-GPU run (SPH_GPUS > 1)"


@pytest.mark.parametrize("slabs", list(SLABS))
def test_a_multi_gpu_run_writes_its_statistics_and_no_frames(sph_run, slabs):
    """The queued click of Simulator::simulate() lands where the single domain's does, and a frame that cannot be
    rendered stops the frames alone: stats.jsonl has the single-GPU run's lines."""
    one = single(sph_run, "stats")
    many = single(sph_run, "stats", **SLABS[slabs])
    assert many.sha() == one.sha()
    assert sorted(many.files) == ["stats.jsonl"] and not [x for x in many.files if x.startswith("frame_")]
    assert len(one.read("stats.jsonl").splitlines()) == FRAMES
    assert many.read("stats.jsonl") == one.read("stats.jsonl")
    assert many.stderr.count(NOT_RENDERED) == 1, many.stderr


@pytest.mark.parametrize("shade,method", [("flat", "renderFrame"), ("speed", "renderField")])
def test_a_multi_gpu_run_refuses_every_other_output_once(sph_run, shade, method):
    many = combined(sph_run, shade, **SLABS["4-loopback"])
    assert sorted(many.files) == ["stats.jsonl"]
    assert many.read("stats.jsonl") == single(sph_run, "stats").read("stats.jsonl")
    assert many.sha() == single(sph_run, "stats").sha()
    lines = [l for l in many.stderr.splitlines() if REFUSED in l]
    methods = [method, "setTracers", "deriveFlow", "labelBodies", "measureBodies", "trackBodies", "neighbourLists", "pairStatistics",
               "sampleField", "extractSurface"]
    assert sorted(l.split(":")[1].strip() for l in lines) == sorted(methods), many.stderr
    assert all(l.startswith("sph: ") for l in lines) and "failed (" not in many.stderr


# ---- 4. SPH_SWEEP=linked with every output ----

def test_the_linked_sweep_refuses_every_walking_output_once(sph_run):
    """SPH_ESTATE: report once, stop that output, go on.  (No click: the linked backend refuses it.  Positions are not
    compared with the list run's: a list's order is a race, tests/test_gpu_linked.py.)"""
    r = sph_run(SPH_SWEEP="linked", **EVERYTHING)
    assert sorted(r.files) == ["frame_%04d.ppm" % f for f in range(FRAMES)] + ["stats.jsonl"]
    assert [json.loads(l)["frame"] for l in r.read("stats.jsonl").splitlines()] == list(range(FRAMES))
    lines = [l for l in r.stderr.splitlines() if "SPH_SWEEP_LINKED" in l]
    methods = ["advectTracers", "deriveFlow", "labelBodies", "measureBodies", "trackBodies", "neighbourLists", "pairStatistics", "sampleField",
               "extractSurface"]
    assert sorted(l.split(":")[1].strip() for l in lines) == sorted(methods), r.stderr
    assert all(l.startswith("sph: ") for l in lines) and "failed (" not in r.stderr
    assert not [l for p in SAID for l in r.said(p)]
