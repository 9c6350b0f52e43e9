"""The tools the sdsp:: headers share (include/sdsp/detail/hip_runtime.h: device_buffer, plan_ptr, host_stage) on their failure
paths: a program compiled with g++ and clang++ under the project's warning flags that does not link libsdsp_hip but defines the few
C functions the detail header calls, with a count of live allocations and a switch that fails the k-th call.  It needs no device."""
import subprocess

import pytest

from conftest import ROOT

SRC = ROOT / "tests" / "cpp" / "test_detail_stage.cpp"
FLAGS = ["-std=c++17", "-O2", "-Wall", "-Wextra", "-Wpedantic", "-Wconversion", "-Werror", f"-I{ROOT / 'include'}"]


@pytest.mark.parametrize("cxx", ["g++", "/opt/rocm/lib/llvm/bin/clang++"])
def test_detail_stage_frees_on_every_path(cxx, tmp_path):
    exe = tmp_path / "test_detail_stage"
    r = subprocess.run([cxx, *FLAGS, str(SRC), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok")
