"""ctypes binding of the reference's own simulator, run on the host (oracle/ref_host/, oracle/Makefile target ref).

TEST INFRASTRUCTURE ONLY, like oracle.py: tests/test_reference_pin_cpu.py and tests/golden/make_golden.py --reference
load it, on a machine that has the reference's sources; nothing else does, and no GPU test.  The library is the
reference's unmodified simulator.cu compiled as C++ (its kernels run serially, one thread after the other) plus a
driver of ours; nothing of it is committed.

What makes a comparison with the oracle exact: the reference's cell lists are built by racing head insertions, so
any order of kernelBuildGrid's threads is an admissible execution.  step(order=ids) runs them in the reverse of
`ids`, so that every list READS in the order of `ids` -- pass OracleSim.sorted_state()["ids"] of the oracle's same
step and the reference sums in the oracle's canonical order; every operation, cut-off, clamp and the click are
then decided by the reference's own text.  Without an order the threads run in descending index: the canonical
order of the first step after setup() or upload().

Hazards, inherited from the reference's text:
 - no bounds check: a particle outside the grid is a wild host write into the cell table.  Only states that stay
   inside the grid may go in; check tests/grid_states.assert_inside on the positions before every step (D = 1:
   one step only, its second step would start outside the grid);
 - setup() with random_init consumes the process's rand(): it equals the unseeded sequence (and
   oracle.init_positions) only as the first consumer in a fresh process.  Run such comparisons in a child process;
 - the reference's destructor frees list nodes that live inside the particle block, so the stand-in's cudaFree is
   a no-op and close() releases the blocks itself; setup() leaks its staging array each time it is called;
 - a click outside the box makes the reference print "OOB particle" lines on stdout.  Nothing may depend on them.
"""
import ctypes as C
import os

import numpy as np

from .oracle import OracleSettings, make_settings

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "_ref", "libsph_reference.so")
_lib = None


def available():
    """whether build() left the reference build (it does where the reference's sources are present)"""
    return os.path.exists(LIB_PATH)


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(LIB_PATH)
        fp, i32p = C.POINTER(C.c_float), C.POINTER(C.c_int32)
        L.ref_create.argtypes = [C.c_void_p, C.c_int]
        L.ref_create.restype = C.c_void_p
        for name in ("ref_setup", "ref_destroy"):
            getattr(L, name).argtypes = [C.c_void_p]
            getattr(L, name).restype = None
        L.ref_upload.argtypes = [C.c_void_p, fp, fp]
        L.ref_set_schedule.argtypes = [C.c_void_p, i32p, C.c_int]
        L.ref_step.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
        L.ref_download.argtypes = [C.c_void_p, fp, fp, fp, fp, fp]
        L.ref_download.restype = None
        L.ref_get_position.argtypes = [C.c_void_p, fp]
        L.ref_get_position.restype = None
        assert L.ref_sizeof_settings() == C.sizeof(OracleSettings), "struct Settings: layout"
        _lib = L
    return _lib


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float)) if a is not None else None


class ReferenceSim:
    """Mirrors OracleSim.  `settings`: any layout-identical Settings struct (grid_states.settings_for); default: the
    reference's own for (n, random_init)."""

    def __init__(self, n, random_init, settings=None):
        self.settings = make_settings(n, random_init)
        if settings is not None:
            assert settings.numParticles == n
            C.memmove(C.byref(self.settings), C.byref(settings), C.sizeof(self.settings))
        self.n = int(n)
        self._is_setup = False
        self._h = lib().ref_create(C.byref(self.settings), C.sizeof(self.settings))
        assert self._h

    def close(self):
        if self._h:
            lib().ref_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def setup(self):
        """the reference's setup(): its allocation and its initialiser"""
        lib().ref_setup(self._h)
        self._is_setup = True

    def upload(self, pos, vel=None):
        """A state in particle-id order, written into particles[] (after the reference's setup(), grid initialiser)."""
        pos = np.ascontiguousarray(pos, dtype=np.float32)
        assert pos.shape == (self.n, 3)
        if vel is not None:
            vel = np.ascontiguousarray(vel, dtype=np.float32)
            assert vel.shape == (self.n, 3)
        if not self._is_setup:
            assert not self.settings.randomInit, "upload() after a random setup(): call setup() yourself"
            self.setup()
        assert lib().ref_upload(self._h, _fp(pos), _fp(vel)) == 0

    def step(self, order=None, click=None):
        """One simulate().  order: particle ids in the order every cell's list must read (see the module docstring).
        click: (x, y) window pixel; the reference's own way -- mouseClicked, clickCoords, then simulate()."""
        assert self._is_setup
        if order is not None:
            order = np.ascontiguousarray(order, dtype=np.int32)
            rc = lib().ref_set_schedule(self._h, order.ctypes.data_as(C.POINTER(C.c_int32)), len(order))
            assert rc == 0, f"schedule refused ({rc}): not a permutation of the particle ids"
        cx, cy = (int(click[0]), int(click[1])) if click is not None else (0, 0)
        assert lib().ref_step(self._h, 1 if click is not None else 0, cx, cy) == 0

    def download(self, want_force=True):
        n = self.n
        out = dict(pos=np.zeros((n, 3), np.float32), vel=np.zeros((n, 3), np.float32), rho=np.zeros(n, np.float32),
                   prs=np.zeros(n, np.float32))
        if want_force:
            out["force"] = np.zeros((n, 3), np.float32)
        lib().ref_download(self._h, _fp(out["pos"]), _fp(out["vel"]), _fp(out["rho"]), _fp(out["prs"]),
                           _fp(out.get("force")))
        return out

    def get_position(self):
        """the reference's getPosition(): the host copy of its last simulate()"""
        out = np.zeros((self.n, 3), np.float32)
        lib().ref_get_position(self._h, _fp(out))
        return out
