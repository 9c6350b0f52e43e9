"""The C++ surface of the LDPC decoder banks (sdsp::ldpc_decoder, include/sdsp/ldpc.h): a program compiled with g++ and clang++
under the project's warning flags; on the GPU it decodes a few noisy codewords of two quasi-cyclic codes, int8 and float input, bytes
and packed bits, in both kernel variants and compares bits, posteriors and status with a direct serial decoder written in the
program."""
import subprocess

import pytest

from conftest import ROOT

SRC = ROOT / "tests" / "cpp" / "test_ldpc.cpp"
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
def test_ldpc_decoder_compiles_warning_free(cxx, tmp_path):
    _compile(cxx, tmp_path / "test_ldpc")


@pytest.mark.gpu
def test_ldpc_decoder_matches_a_direct_decoder_on_gpu(tmp_path):
    exe = _compile("g++", tmp_path / "test_ldpc")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok")
