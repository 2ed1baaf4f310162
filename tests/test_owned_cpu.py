"""The owning types of csrc/sph_owned.h (DeviceBuf, PinnedBuf, Event) without a GPU: tests/owned_selftest.cpp defines
the six HIP functions the header calls as counting fakes over malloc / free, runs under the host sanitizers as a
stand-alone program, and prints what it counted.  Logs: m / f a device allocation / release, M / F pinned, c / d an
event created / destroyed, x a call the fake refused."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


@pytest.fixture(scope="module")
def selftest(tmp_path_factory):
    """tests/owned_selftest.cpp under ASan + UBSan, run once: {name: [values]}"""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("owned") / "owned_selftest")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROCM, "include"),
                    "-I", os.path.join(ROOT, "cudafluidsimulator_amd", "csrc"),
                    os.path.join(ROOT, "tests", "owned_selftest.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0 and not p.stderr, f"sanitizer report or failure:\n{p.stderr}"
    out = {}
    for line in p.stdout.splitlines():
        name, val = line.split()
        out.setdefault(name, []).append(val)
    return out


def test_every_allocation_is_released_once_at_scope_exit(selftest):
    assert selftest["scope_rc"] == ["0"] * 4
    assert selftest["scope_dev_bytes"] == ["80"] and selftest["scope_pin_bytes"] == ["28"]  # count x sizeof(T)
    assert selftest["scope_pin_mapped"] == selftest["scope_pin_default"] == selftest["scope_evt_flags"] == ["1"]
    assert selftest["scope_converts"] == ["1"]
    assert selftest["scope_log"] == ["mMFMcdFf"] and selftest["scope_live"] == ["0"]


def test_alloc_on_a_full_object_releases_the_old_block_first(selftest):
    assert selftest["again_rc"] == ["0"] * 4
    assert selftest["again_log"] == ["mfmMFMFf"] and selftest["again_live"] == ["0"]


def test_a_failed_alloc_leaves_the_object_empty(selftest):
    assert selftest["fail_rc_before"] == ["0"] and selftest["fail_rc_after"] == ["0"]
    assert selftest["fail_dev_refused"] == selftest["fail_pin_refused"] == selftest["fail_evt_refused"] == ["1"]
    assert selftest["fail_empty"] == ["1"]
    # the old blocks go before the refused calls and are not released again at scope exit
    assert selftest["fail_log"] == ["mMfxFxxmf"] and selftest["fail_live"] == ["0"]


def test_moves_leave_the_source_empty_and_the_totals_balanced(selftest):
    assert selftest["move_rc"] == ["0"]
    for name in ("ctor_source_empty", "ctor_target_holds", "assign_source_empty", "assign_target_holds", "self_keeps"):
        assert selftest["move_" + name] == ["1"], name
    # construction calls nothing; assignment releases the target's own block; scope exit the three that are left
    assert selftest["move_log"] == ["mmMMcc|fFd|dFf"] and selftest["move_live"] == ["0"]


def test_reset_on_an_empty_object_calls_nothing(selftest):
    assert selftest["reset_empty_log"] == ["-"] and selftest["reset_empty_live"] == ["0"]
    assert selftest["reset_rc"] == ["0"] and selftest["reset_leaves_empty"] == ["1"]
    assert selftest["reset_log"] == ["mMcfFd"] and selftest["reset_live"] == ["0"]


def test_event_create_twice_creates_once(selftest):
    assert selftest["twice_rc"] == ["0", "0"] and selftest["twice_same"] == ["1"]
    assert selftest["twice_log"] == ["cd"] and selftest["twice_live"] == ["0"]


def test_the_step_rings_shape_balances(selftest):
    assert selftest["ring_rc"] == ["0"]
    assert selftest["ring_created"] == selftest["ring_live_inside"] == [str(64 * 8)]
    assert selftest["ring_live"] == ["0"]


def test_totals(selftest):
    one = lambda name: int(selftest[name][0])
    assert one("total_dev_made") == one("total_dev_released") == 8
    assert one("total_pin_made") == one("total_pin_released") == 8
    assert one("total_evt_made") == one("total_evt_released") == 5 + 64 * 8
    assert one("total_unknown_releases") == 0
