"""The buffer choice of the coverage pass (csrc/cover_pool.hpp: pick_cover_buffer) on the CPU: tests/cover_pool_model.cpp is compiled with the host compiler as a
stand-alone program -- once plainly, once with AddressSanitizer and UndefinedBehaviorSanitizer -- and run directly.  Nothing is loaded into Python.

The program drives the choice through scripted sequences over a small model of the streams (frames of a stream complete in order, when the script says so) and
checks after every pick that a busy buffer only ever goes back to its own stream, with `wait` set, and that it is that stream's OLDEST frame in flight:
  * one stream hundreds of frames ahead of the GPU alternates between two buffers and never waits for its newest frame; with the GPU one frame behind it never
    waits at all; with one buffer per stream (the deliberately slow form) every launch waits for the newest;
  * twelve streams over eight buffers: eight are served, four are refused (-1) until frames complete;
  * completions in every order (all 2520 orders of two frames on each of four streams), and random interleavings of launches and completions over pools of 1 to 8
    buffers and 1 to 12 streams;
  * an exhausted pool gives -1, and a buffer again once some frame has completed."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cover_pool_model.cpp")
INC = os.path.join(ROOT, "rust-ray-tracer_amd", "csrc")
N_RUNS = 2000                 # random interleavings of the plain build
N_SANITIZED = 300             # the instrumented build runs the same program on fewer: it checks the program's memory and arithmetic


def _build_and_run(tmp_path, name, extra_flags, n):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = os.path.join(str(tmp_path), name)
    subprocess.run([cxx, "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", *extra_flags, "-I", INC, "-o", exe, SRC], check=True)
    run = subprocess.run([exe, str(n)], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    return {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", run.stdout.strip().splitlines()[-1])}


def test_model_sequences(tmp_path):
    out = _build_and_run(tmp_path, "cover_pool_model", [], N_RUNS)
    assert out["failures"] == 0
    assert out["picks"] >= 100_000 and out["waits"] >= 10_000 and out["refusals"] >= 1_000, out      # every outcome of the choice was reached, often


def test_model_sequences_sanitized(tmp_path):
    out = _build_and_run(tmp_path, "cover_pool_model_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], N_SANITIZED)
    assert out["failures"] == 0 and out["picks"] >= 50_000, out
