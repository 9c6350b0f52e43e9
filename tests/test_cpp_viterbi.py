"""The C++ surface of the Viterbi decoder banks (sdsp::viterbi_bank, include/sdsp/viterbi.h): a program compiled with g++ and clang++
under the project's warning flags; on the GPU it decodes 5 channels of the K = 7 (171, 133) code in both kernel variants and of a K = 5
rate-1/3 code, int8 and float soft values, bytes and packed words, in two calls, and compares bits and final metrics with a direct loop
written in the program."""
import subprocess

import pytest

from conftest import ROOT

SRC = ROOT / "tests" / "cpp" / "test_viterbi.cpp"
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
def test_viterbi_bank_compiles_warning_free(cxx, tmp_path):
    _compile(cxx, tmp_path / "test_viterbi")


@pytest.mark.gpu
def test_viterbi_bank_matches_direct_loops_on_gpu(tmp_path):
    exe = _compile("g++", tmp_path / "test_viterbi")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok")
