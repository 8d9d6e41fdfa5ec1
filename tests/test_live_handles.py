"""The registry of live handles (csrc/live_handles.hpp) and the Python base of the handle wrappers (host._Handle): the
header under the sanitizers in a stand-alone program, the base class against a stub library that records its calls."""
import functools
import os
import subprocess
import tempfile
import warnings

import pytest

from opencalibration_amd import capi, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(None)
def driver(sanitizers):
    """tests/live_handles_driver.cpp built with -fsanitize=<sanitizers>; without where the runtime does not link.
    Returns (path, sanitized)."""
    exe = os.path.join(tempfile.mkdtemp(prefix="live_handles_driver_"), "live_handles_driver")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-pthread", "-o", exe, os.path.join(ROOT, "tests", "live_handles_driver.cpp")]
    if subprocess.run(cmd + ["-fsanitize=" + sanitizers, "-fno-sanitize-recover=all"], capture_output=True).returncode == 0:
        return exe, True
    subprocess.run(cmd, check=True)
    return exe, False


@pytest.mark.parametrize("sanitizers", ["address,undefined", "thread"])
def test_live_set_in_a_standalone_program(sanitizers):
    """nullptr, unknown, add / has / remove once, two types over one address, and 8 threads of 10 000 objects each beside a
    poller: the program checks its own answers and ends clean under the sanitizers"""
    exe, sanitized = driver(sanitizers)
    if not sanitized:
        warnings.warn(f"the {sanitizers} sanitizer runtime does not link here: the stand-alone program ran without -fsanitize")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-2000:] + r.stderr[-4000:]


class StubLibrary:
    """what _Handle asks of a library: a destroy and a last-error function, by name; the calls are recorded"""

    def __init__(self):
        self.destroyed = []

    def stub_destroy(self, h):
        self.destroyed.append(h)

    def stub_last_error(self):
        return b"stub: refused"


class StubContext:
    h = 7


class Stub(host._Handle):
    _destroy, _last_error = "stub_destroy", "stub_last_error"

    def __init__(self, lib, ctx=None, fail=False):
        self.L, self.ctx, self.released = lib, ctx, 0
        if fail:
            raise RuntimeError("before h was set")
        self.h = 41

    def _released(self):
        self.released += 1


def test_handle_close_twice_destroys_once():
    lib = StubLibrary()
    s = Stub(lib)
    s.close()
    assert lib.destroyed == [41] and s.h is None and s.released == 1
    s.close()
    assert lib.destroyed == [41] and s.h is None
    del s                                                   # the collector closes once more: still one destroy
    assert lib.destroyed == [41]


def test_handle_skips_the_destroy_after_its_context():
    lib, ctx = StubLibrary(), StubContext()
    s = Stub(lib, ctx)
    ctx.h = None                                            # the context was closed first
    s.close()
    assert lib.destroyed == [] and s.h is None and s.released == 1
    live = Stub(lib, StubContext())                         # a context that is still open: destroyed
    live.close()
    assert lib.destroyed == [41]


def test_handle_exit_closes():
    lib = StubLibrary()
    with Stub(lib) as s:
        assert s.h == 41 and lib.destroyed == []
    assert lib.destroyed == [41] and s.h is None


def test_handle_closes_after_a_failed_init():
    lib = StubLibrary()
    s = Stub.__new__(Stub)
    with pytest.raises(RuntimeError):
        s.__init__(lib, fail=True)
    s.close()
    assert lib.destroyed == [] and s.h is None and s.released == 1
    bare = Stub.__new__(Stub)                               # __init__ raised before anything was set
    bare.released = 0
    bare.close()
    assert bare.h is None


def test_handle_check():
    s = Stub(StubLibrary())
    assert s._check(0) == 0
    with pytest.raises(capi.OchipError, match="stub: refused"):
        s._check(-1)
