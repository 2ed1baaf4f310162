"""Random sequences of steps, state changes and all fourteen analysis passes on one handle, held to a model
(tests/pass_sequences.py): the state to the oracle after every state operation, every pass result to its restatement
at the moment of the call -- fed by sph_download_state + sph_download_grid taken after the call, through the helpers of
the passes' own test files --, every refusal to what it must leave alone, every host reader to the copy taken at the
call, and the run's final state to that of a handle that made the same state operations and no pass call.  Off the
100^3 grid: D7, D10h025, D41 and D102 of tests/grid_states.py, one sort plan each.  Every comparison is of words.
tests/test_pass_sequences_cpu.py shows what the seed list covers.  Measured on an MI355X: the 24 seeds and the knob
check take 27.8 s, the costliest seed (23, D102) 3.2 s, every other under 2.8 s.

The rules the readers are held to ("What a result outlives"):
  * a host reader serves the last successful call of its pass until the next call of that pass, across steps, clicks,
    uploads, loads and every other pass;
  * sph_bodies_host serves the labelling of whichever of sph_label_bodies, sph_measure_bodies and sph_track_bodies ran
    last -- a call refused by max_bodies or max_edges included: it labelled before it was refused;
  * a refused call leaves no result of its own: sph_body_moments_host, sph_body_tracks_host, sph_neighbours_host are
    SPH_ESTATE after it, and so is sph_body_tracks_host after sph_track_reset;
  * a call refused for its arguments is another matter: sph_pair_statistics with 129 bins or a radius above h is
    SPH_EINVAL before it touches anything, and sph_pair_statistics_host goes on serving the previous result (SPH_ESTATE
    where there was none);
  * the device-side readers (sph_download_frame_buffers and the like) are read at the call only."""
import ctypes as C

import numpy as np
import pytest

import cudafluidsimulator_amd as sph
from cudafluidsimulator_amd import _lib

import body_tracks_restatement as T
import diagnostics_restatement as D
import pair_restatement as PR
import grid_states as G
import pass_sequences as PS
import test_gpu_api_fuzz as FZ
import test_gpu_bodies as TB
import test_gpu_body_moments as TM
import test_gpu_column_frame as TC
import test_gpu_derived as TD
import test_gpu_field_frame as TF
import test_gpu_liquid_frame as TL
import test_gpu_neighbours as TN
import test_gpu_render as TR
from helpers import assert_bit_equal

pytestmark = pytest.mark.gpu

F = np.float32
BODY_KEYS = ("labels", "table", "num_bodies", "largest")
TRACK_KEYS = ("tracks", "previous", "edges", "summary")


def test_the_knobs_are_the_existing_fuzzs():
    assert PS.KNOBS == FZ.KNOBS


class tagged:
    """inside: an SphError of code `rc` must be raised; everything else, a missing error included, fails with the tag"""

    def __init__(self, tag, rc):
        self.tag, self.rc = tag, rc

    def __enter__(self):
        return self

    def __exit__(self, kind, e, tb):
        if kind is None:
            raise AssertionError(f"{self.tag}: no error, SphError ({self.rc}) expected")
        if not issubclass(kind, sph.SphError):
            return False
        assert f"({self.rc})" in str(e), f"{self.tag}: SphError ({self.rc}) expected, got: {e}"
        return True


class Bare:
    """a handle that makes a plan's state operations"""

    def __init__(self, p, model, tmp_path, who):
        pos, vel = model.start
        self.sim = sph.Simulator(G.settings_for(len(pos), model.g["h"], model.g["cells"], factory=sph.default_settings), sweep=p["sweep"])
        self.sim.upload_state(pos, vel)
        self.times = sph.Times()
        self.tmp, self.who = tmp_path, who

    def apply(self, op, model, k):
        sim, kind = self.sim, op["kind"]
        if kind == "step":
            sim.simulate()
        elif kind == "timed":
            sim.simulateAndTime(self.times)
        elif kind == "click":
            sim.mouseClicked, sim.clickCoords = True, op["pixel"]
            sim.simulate()
        elif kind == "upload":
            sim.upload_state(*model.upload_of(op))
        else:
            assert kind == "snapshot", kind
            path = self.tmp / f"{self.who}{k}.sphsnap"
            sim.save_state(path)
            sim.simulate()                      # (moves on, then comes back to the snapshot)
            sim.load_state(path)

    def phase(self, name):
        self.sim.phase(name)

    def final(self):
        st = self.sim.download_state()
        st["host"] = np.array(self.sim.getPosition(), copy=True)
        return st

    def close(self):
        self.sim.close()


class Device(Bare):
    """the handle under test: the passes, the refusals and the readers as well"""

    def __init__(self, p, model, tmp_path, monkeypatch):
        super().__init__(p, model, tmp_path, "dev")
        self.model, self.mp = model, monkeypatch
        self.last = dict.fromkeys(PS.READERS)

    def check(self, model, tag):
        FZ.check(self.sim, model.ref, tag)

    def inputs(self, walked):
        """walked: the call walked the grid, sph_download_grid returns it; else the state over a grid built on the CPU
        (which the restatements of such a call do not read)"""
        st = self.sim.download_state()
        if walked:
            g = self.sim.download_grid()
            return PS.Inputs(st, g["ids"], g["cells"])
        _, ids, cells = PS.NR.grid_of(st["pos"], self.model.h, self.model.D)
        return PS.Inputs(st, ids, cells)

    def helpers(self):
        sim = self.sim
        return {"derive": lambda: TD.restate(sim), "bodies": lambda link: TB.restate(sim, link), "walk": lambda r: TN.walk_of(sim, r)}

    # -- the passes --
    def call(self, op, iso):
        sim, kind = self.sim, op["kind"]
        self.mp.setenv(PS.PLAIN[kind], op["plain"])
        if kind in PS.FRAMES:
            size = dict(width=op["size"][0], height=op["size"][1])
        if kind == "flat":
            return TR.gpu_frame(sim, point_size=op["point_size"], shade=op["shade"], **size)
        if kind == "field":
            got = TF.gpu_field(sim, field=op["field"], lo=op["range"][0], hi=op["range"][1], point_size=op["point_size"], **size)
        elif kind == "column":
            got = TC.gpu_column(sim, lo=op["range"][0], hi=op["range"][1], **size)
        if kind in ("field", "column"):
            got["range"] = np.array(got["range"], F)
            return got
        if kind == "liquid":
            return TL.gpu_liquid(sim, smooth_iterations=op["smooth"], **size)
        if kind == "sample":
            got = dict(field=sim.sample_field(op["field"], *PS.lattice(self.model.g, op["shape"])))
            got["dims"] = self.read("sample", dims_only=True)
            return got
        if kind == "surface":
            return sim.extract_surface(iso, *PS.lattice(self.model.g, op["shape"]))
        if kind == "diagnose":
            sim.diagnose(op["hist"], op["value_range"])
            return dict(raw=sim.diagnostics_raw())
        if kind == "tracers":
            if op["set"] is not None:
                sim.set_tracers(self.model.tracers_of(op))
            sim.advect_tracers(op["dt"])
            return sim.tracers()
        if kind == "derive":
            return sim.derive()
        if kind == "lists":
            return sim.neighbour_lists(op["radius"], walk_order=op["walk_order"])
        if kind == "pairs":
            self.mp.setenv("SPH_PAIRS_WORKGROUPS", op["workgroups"])
            return sim.pair_statistics(op["bins"], op["radius"])
        if kind == "label":
            return sim.label_bodies(op["link"])
        if kind == "measure":
            return sim.measure_bodies(op["link"])
        assert kind == "track", kind
        return sim.track_bodies(op["link"], moments=op["moments"])

    def compare(self, op, got, want, tag):
        kind, last = op["kind"], self.last
        if kind == "diagnose":
            D.assert_same_words(got["raw"], D.to_struct(want["raw"]), tag)
            last["diagnose"] = bytes(got["raw"])
            return
        if kind == "pairs":
            # the table as Python ints, then the raw rows and edges word for word (as test_gpu_pairs.both_paths)
            PR.assert_same_table(got, want, tag)
            assert got["edges2"].dtype == F and got["pairs"].dtype == np.uint64, tag
            assert PR.describe_difference(PR.from_rows(got["rows"], got["edges2"]), want) == [], tag
            assert got["rows"].tobytes() == PR.to_rows(want).tobytes() and got["edges2"].tobytes() == want["edges2"].tobytes(), tag
            last["pairs"] = dict(rows=got["rows"].copy(), edges2=got["edges2"].copy(), bins=len(got["rows"]))
            return
        if kind == "track":
            join = want.pop("join")
            T.assert_same(got, join, tag)
            assert np.array_equal(got["table"][:, 0], join["labels"]) and np.array_equal(got["table"][:, 1], join["counts"]), tag
            last["tracks"] = {k: got[k] for k in TRACK_KEYS}
        PS.assert_same(got, want, tag)
        if kind in PS.FRAMES:
            last["frame"] = got["rgb"]
        elif kind == "sample":
            last["sample"] = got["field"]
        elif kind in ("surface", "tracers", "derive", "lists"):
            last[kind] = got
        else:
            last["bodies"] = {k: got[k] for k in BODY_KEYS}
            if "moments" in got:
                TM.assert_same_moments(got, TM.M.from_rows(want["moments"]), tag)
                last["moments"] = {k: got[k] for k in ("moments", "size_hist")}

    # -- the refusals --
    def refuse(self, op, tag):
        sim = self.sim
        if op["what"] == "pair_options":
            self.mp.setenv("SPH_PAIRS_PLAIN", op["plain"])
            with tagged(tag, -1):
                sim.pair_statistics(op["bins"], op["radius"])
            return
        link = op["link"]
        self.mp.setenv("SPH_BODIES_PLAIN", op["plain"])
        self.mp.setenv("SPH_NEIGHBOURS_PLAIN", op["plain"])
        with tagged(tag, -3):
            if op["what"] == "max_edges":
                sim.track_bodies(link, max_edges=1, moments=op["moments"])
            elif op["what"] == "max_bodies":
                sim.measure_bodies(link, max_bodies=1)
            else:
                sim.neighbour_lists(link, max_entries=1)

    def refused(self, op, labelling, tag):
        """after a refusal: the labelling it made is the one sph_bodies_host serves, its own reader has nothing"""
        last = self.last
        if op["what"] == "pair_options":
            # SPH_EINVAL took nothing: the previous table is still served, word for word
            if last["pairs"] is None:
                with tagged(f"{tag}: pairs read after the refusal, with no result before it", -4):
                    self.read("pairs")
            else:
                self.reread("pairs", f"{tag}: sph_pair_statistics_host after the refusal")
            return
        if op["what"] == "max_entries":
            last["lists"] = None
            gone = ["lists"]
        else:
            got = self.read("bodies")
            PS.assert_same(got, labelling, f"{tag}: sph_bodies_host after the refusal")
            last["bodies"] = got
            gone = ["tracks"] if op["what"] == "max_edges" else ["moments"]
            if op["what"] == "max_edges" and op["moments"]:
                gone.append("moments")
        for reader in gone:
            last[reader] = None
            with tagged(f"{tag}: {reader} read after the refusal", -4):
                self.read(reader)

    def probe(self, op, tag):
        """a pass in phase 2 or 3: SPH_ESTATE"""
        with tagged(tag, -4):
            self.call(op, 1.0)

    def reset(self, tag):
        self.sim.track_reset()
        self.last["tracks"] = None
        with tagged(f"{tag}: sph_body_tracks_host after the reset", -4):
            self.read("tracks")

    # -- the host readers --
    def read(self, reader, dims_only=False):
        sim = self.sim
        L, h, ck = sim._L, sim._h, sim._check
        rows = sph.simulator._rows
        if reader == "frame":
            return np.array(sim.frame_host(), copy=True)
        if reader == "sample":
            nx, ny, nz = C.c_int(0), C.c_int(0), C.c_int(0)
            p = L.sph_sample_host(h, C.byref(nx), C.byref(ny), C.byref(nz))
            if not p:
                raise sph.SphError("sph_sample_host failed (-4): " + L.sph_last_error(h).decode())
            dims = (nz.value, ny.value, nx.value)       # the lattice the reader reports shapes what is read
            return dims if dims_only else np.array(np.ctypeslib.as_array(p, shape=dims), copy=True)
        if reader == "surface":
            vp, tp, nv, nt = C.POINTER(C.c_float)(), C.POINTER(C.c_uint32)(), C.c_int64(0), C.c_int64(0)
            ck(L.sph_surface_host(h, C.byref(vp), C.byref(nv), C.byref(tp), C.byref(nt)), "sph_surface_host")
            return {"vertices": rows(vp, nv.value, 3, np.float32), "triangles": rows(tp, nt.value, 3, np.uint32)}
        if reader == "diagnose":
            return bytes(sim.diagnostics_raw())
        if reader == "tracers":
            return sim.tracers()
        if reader == "derive":
            wd, gr, nb, n = C.POINTER(C.c_float)(), C.POINTER(C.c_float)(), C.POINTER(C.c_uint32)(), C.c_int(0)
            ck(L.sph_derived_host(h, C.byref(wd), C.byref(gr), C.byref(nb), C.byref(n)), "sph_derived_host")
            wd, gr = rows(wd, n.value, 4, np.float32), rows(gr, n.value, 4, np.float32)
            return dict(vorticity=np.ascontiguousarray(wd[:, :3]), divergence=np.ascontiguousarray(wd[:, 3]),
                        grad_rho=np.ascontiguousarray(gr[:, :3]), rho=np.ascontiguousarray(gr[:, 3]), neighbours=rows(nb, n.value, None, np.uint32))
        if reader == "lists":
            off, nb, n, entries = C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint32)(), C.c_int(0), C.c_uint64(0)
            ck(L.sph_neighbours_host(h, C.byref(off), C.byref(nb), C.byref(n), C.byref(entries)), "sph_neighbours_host")
            return dict(offsets=rows(off, n.value + 1, None, np.uint64), neighbours=rows(nb, entries.value, None, np.uint32))
        if reader == "bodies":
            lab, tab, n, k, big = C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint32)(), C.c_int(0), C.c_int(0), C.c_uint32(0)
            ck(L.sph_bodies_host(h, C.byref(lab), C.byref(n), C.byref(tab), C.byref(k), C.byref(big)), "sph_bodies_host")
            return dict(labels=rows(lab, n.value, None, np.uint32), table=rows(tab, k.value, 8, np.uint32), num_bodies=k.value, largest=big.value)
        if reader == "moments":
            p, m, hist = C.POINTER(_lib.SphBodyMomentsRaw)(), C.c_int(0), C.POINTER(C.c_uint32)()
            ck(L.sph_body_moments_host(h, C.byref(p), C.byref(m), C.byref(hist)), "sph_body_moments_host")
            w = rows(C.cast(p, C.POINTER(C.c_uint64)), m.value, C.sizeof(_lib.SphBodyMomentsRaw) // 8, np.uint64)
            return dict(moments=w.view(_lib.body_moments_dtype()).reshape(-1), size_hist=rows(hist, _lib.BODY_SIZE_BINS, None, np.uint32))
        if reader == "pairs":
            pr, ed, b = C.POINTER(_lib.SphPairBinRaw)(), C.POINTER(C.c_float)(), C.c_int(-1)
            ck(L.sph_pair_statistics_host(h, C.byref(pr), C.byref(ed), C.byref(b)), "sph_pair_statistics_host")
            w = rows(C.cast(pr, C.POINTER(C.c_uint64)), b.value, C.sizeof(_lib.SphPairBinRaw) // 8, np.uint64)
            return dict(rows=w.view(_lib.pair_bin_dtype()).reshape(-1), edges2=rows(ed, b.value, None, np.float32), bins=b.value)
        assert reader == "tracks", reader
        tr, fa, ed = C.POINTER(_lib.SphBodyTrack)(), C.POINTER(_lib.SphBodyFate)(), C.POINTER(_lib.SphBodyEdge)()
        nt, nf, ne, summ = C.c_int(0), C.c_int(0), C.c_int(0), _lib.SphBodyTrackSummary()
        ck(L.sph_body_tracks_host(h, C.byref(tr), C.byref(nt), C.byref(fa), C.byref(nf), C.byref(ed), C.byref(ne), C.byref(summ)), "sph_body_tracks_host")
        structs = lambda p, count, struct, dtype: rows(C.cast(p, C.POINTER(C.c_uint32)), count, C.sizeof(struct) // 4, np.uint32).view(dtype).reshape(-1)
        return dict(tracks=structs(tr, nt.value, _lib.SphBodyTrack, _lib.body_track_dtype()),
                    previous=structs(fa, nf.value, _lib.SphBodyFate, _lib.body_fate_dtype()),
                    edges=structs(ed, ne.value, _lib.SphBodyEdge, _lib.body_edge_dtype()),
                    summary={name: int(getattr(summ, name)) for name in _lib.TRACK_SUMMARY})

    def reread(self, reader, tag):
        """the last result of a pass through its host reader again: the copy taken at the call (the plans read only
        readers that hold one)"""
        want = self.last[reader]
        assert want is not None, f"{tag}: the plan reads a reader that holds nothing"
        try:
            got = self.read(reader)
        except sph.SphError as e:
            raise AssertionError(f"{tag}: the reader no longer serves the last result: {e}") from e
        if isinstance(want, dict):
            want = {k: (np.array(sorted(v.items())) if isinstance(v, dict) else v) for k, v in want.items()}
            got = {k: (np.array(sorted(v.items())) if isinstance(v, dict) else v) for k, v in got.items()}
            PS.assert_same(got, want, f"{tag}: read again")
        elif isinstance(want, bytes):
            assert got == want, f"{tag}: read again"
        else:
            PS.assert_same(dict(result=got), dict(result=want), f"{tag}: read again")


def run(p, monkeypatch, tmp_path):
    for k, v in p["env"].items():
        monkeypatch.setenv(k, v)
    model, handles = PS.Model(p), []
    try:
        device = Device(p, model, tmp_path, monkeypatch)
        handles.append(device)
        bare = Bare(p, model, tmp_path, "bare")
        handles.append(bare)
        PS.drive(p, model, device, bare)
        got, want = device.final(), bare.final()
        for k in want:
            assert_bit_equal(got[k], want[k], f"seed {p['seed']} ({p['grid']}, {p['sweep']}), after op {len(p['ops']) - 1} "
                                              f"{PS.describe(p['ops'][-1])}: {k} at the end against the handle that called no pass")
    finally:
        for d in handles:
            d.close()
        model.close()


@pytest.mark.parametrize("seed", PS.SEEDS)
def test_random_sequences_of_passes_stay_on_the_model(seed, monkeypatch, tmp_path):
    run(PS.plan(seed), monkeypatch, tmp_path)
