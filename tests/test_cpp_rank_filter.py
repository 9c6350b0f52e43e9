"""The C++ surface of the rank-order filter bank (sdsp::rank_filter_bank, include/sdsp/rank_filter.h): a program compiled with g++ and
clang++ under the project's warning flags; on the GPU it streams sines with isolated impulses through a 5-point median in blocks and
checks that every output equals a std::nth_element loop computed in the program, bit for bit, and that no impulse survives."""
import subprocess

import pytest

from conftest import ROOT

SRC = ROOT / "tests" / "cpp" / "test_rank_filter.cpp"
FLAGS = ["-std=c++17", "-O2", "-Wall", "-Wextra", "-Wpedantic", "-Wconversion", "-Werror", f"-I{ROOT / 'include'}"]


def _compile(cxx, out):
    import simpledsp_amd
    simpledsp_amd.load()  # builds libsdsp_hip.so if needed
    lib = ROOT / "simpledsp_amd" / "lib"
    out.parent.mkdir(parents=True, exist_ok=True)
    r = subprocess.run([cxx, *FLAGS, str(SRC), "-o", str(out), f"-L{lib}", "-lsdsp_hip", f"-Wl,-rpath,{lib}",
                        "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return out


@pytest.mark.parametrize("cxx", ["g++", "/opt/rocm/lib/llvm/bin/clang++"])
def test_rank_filter_bank_compiles_warning_free(cxx, tmp_path):
    _compile(cxx, tmp_path / "test_rank_filter")


@pytest.mark.gpu
def test_rank_filter_bank_removes_impulses_on_gpu(tmp_path):
    exe = _compile("g++", tmp_path / "test_rank_filter")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok")
