"""Scaffolding of the ABI tests, which need no GPU: the stand-ins for the library and for device tensors that show what the Python binding does before it calls
the library (NoLibrary, CallRecorder, fake_device, bare_raytracer), the loop over calls the library has to refuse (assert_refused), and the size and offsets the
header's own compiler gives a struct (compiled_layout; compiled_values for any integer expressions of the header, such as enum constants).

Plain module, not a test module: pytest does not rewrite its asserts, so every assert here states both values in its message.  It holds no fixtures.
"""
import shutil
import subprocess

import numpy as np

from bitwise import same
from conftest import ROOT

PATTERN = 0xA5A5A5A5                                  # what the outputs of a call that has to be refused are filled with


class NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name}) with arguments the binding has to refuse")


class CallRecorder:
    """A library whose every entry point records (name, args) and returns RRT_OK."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            return 0
        return entry


def fake_device(t, device=None):
    """What the binding's _device_tensor asks of a tensor, with is_cuda forced (and, when given, `device`): its contiguity, dtype and length checks can then be
    reached without a GPU."""
    class FakeDeviceTensor:
        is_cuda = True

        def __getattr__(self, k):
            return getattr(t, k)
    if device is not None:
        FakeDeviceTensor.device = device
    return FakeDeviceTensor()


def bare_raytracer(rrt):
    rt = rrt.RayTracer.__new__(rrt.RayTracer)                                # no handle: nothing may get as far as needing one
    rt._h = None
    return rt


def assert_refused(rrt, L, calls, untouched=()):
    """Every (what, call) of `calls` returns RRT_ERR_INVALID_ARG and sets an error detail of its own -- another failure's detail is set first, so that a detail left
    unchanged would show -- and every array of untouched ({name: array}) still holds what it held before the calls."""
    untouched = dict(untouched)
    before = {name: np.array(a, copy=True) for name, a in untouched.items()}
    for what, call in calls:
        assert L.rrt_host_buffer_register(None, 0) == rrt.ERR_INVALID_ARG, f"{what}: the other failure was not refused"
        other = L.rrt_last_error_detail()
        status = call()
        assert status == rrt.ERR_INVALID_ARG, f"{what}: status {status}, want {rrt.ERR_INVALID_ARG}"
        assert L.rrt_last_error_detail() not in (b"", None, other), f"{what}: the error detail is {L.rrt_last_error_detail()!r} after {other!r}"
        for name, a in untouched.items():
            assert same(a, before[name]), f"{what}: {name} of a refused call was written"


def host_compiler():
    """The host C compiler build() itself needs (for the oracle), or None."""
    return shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")


def compiled_values(tmp_path, expressions):
    """The values of integer C expressions (sizeof, offsetof, enum constants) as a program compiled against include/rrt.h prints them."""
    cc = host_compiler()
    assert cc is not None, "no host C compiler (build() needs one for the oracle)"
    src = tmp_path / "values.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "rrt.h"\nint main(void) {\n'
                   + "".join(f'    printf("%lld\\n", (long long)({e}));\n' for e in expressions) + "    return 0;\n}\n")
    subprocess.run([cc, "-std=c99", "-I", f"{ROOT}/include", "-o", str(tmp_path / "values"), str(src)], check=True)
    got = [int(v) for v in subprocess.run([str(tmp_path / "values")], check=True, capture_output=True, text=True).stdout.split()]
    assert len(got) == len(expressions), f"{len(got)} values for {len(expressions)} expressions"
    return got


def compiled_layout(tmp_path, struct, fields):
    """(size of the header's struct, [offset of each of `fields`]) by the header's own compiler."""
    size, *offsets = compiled_values(tmp_path, [f"sizeof({struct})"] + [f"offsetof({struct}, {f})" for f in fields])
    return size, offsets
