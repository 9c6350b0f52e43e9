"""The C++ surface of the Reed-Solomon decoder banks (sdsp::rs_decoder, include/sdsp/rs.h): a program compiled with g++ and clang++
under the project's warning flags; on the GPU it decodes a few frames of RS(255, 223) at I = 5 with erasure flags and of the shortened
RS(204, 188) in both kernel variants and compares bytes and counts with a direct serial decoder written in the program."""
import subprocess

import pytest

from conftest import ROOT

SRC = ROOT / "tests" / "cpp" / "test_rs.cpp"
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
def test_rs_decoder_compiles_warning_free(cxx, tmp_path):
    _compile(cxx, tmp_path / "test_rs")


@pytest.mark.gpu
def test_rs_decoder_matches_a_direct_decoder_on_gpu(tmp_path):
    exe = _compile("g++", tmp_path / "test_rs")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok")
