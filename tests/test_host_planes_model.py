"""The pure part of the host forms (csrc/host_planes.hpp) on the CPU: tests/host_planes_model.cpp is compiled with the host compiler as a stand-alone
program -- once plainly, once with AddressSanitizer and UndefinedBehaviorSanitizer -- and run directly.  No GPU, no HIP header: the header must compile
with -Wall -Wextra -Werror from include/rrt.h and the C++ library alone.

The program carves plane lists out of a fake arena address and checks: every table of bytes per entry against sizeof of its public pointer struct and
against the element type rrt.h declares for each field; planes_bytes and carve_planes (null planes take nothing, wanted ones sit in list order at
multiples of 256, an empty one has an address of its own, the total is the sum of the slots); the mirrored device struct of each of the seven structs,
for the full set and for each field alone, and of a struct that lies in two runs of a list; the rule of ray_set_planes that an array named twice goes up
once (src.origins == src.rec.next_origin, src.dirs == src.rec.next_dir: two uploads, not four) and that equal pointers of different element sizes do
not alias; the traced pixels and the ray batches of a region with the numbers of tests/test_gpu_launch_paths.py, and the refusals of a region and an order."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_planes_model.cpp")
INC = os.path.join(ROOT, "rust-ray-tracer_amd", "csrc")


def _build_and_run(tmp_path, name, extra_flags):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = os.path.join(str(tmp_path), name)
    subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", *extra_flags, "-I", INC, "-o", exe, SRC], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    fields = dict(re.findall(r"(\w+)=(\d+)", run.stdout.strip().splitlines()[-1]))
    return {k: int(v) for k, v in fields.items()}


def test_host_planes_model(tmp_path):
    out = _build_and_run(tmp_path, "host_planes_model", [])
    assert out["failures"] == 0 and out["checks"] >= 1000, out


def test_host_planes_model_sanitized(tmp_path):
    out = _build_and_run(tmp_path, "host_planes_model_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    assert out["failures"] == 0 and out["checks"] >= 1000, out
