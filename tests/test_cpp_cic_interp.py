"""The C++ surface of the CIC interpolator bank (sdsp::cic_interpolator_bank, include/sdsp/cic_interp.h): a program compiled with g++
and clang++ under the project's warning flags; on the GPU it streams blocks of irregular length through the bank and checks every
channel, bit for bit, against a serial Hogenauer loop written in the program."""
import subprocess

import pytest

from conftest import ROOT

SRC = ROOT / "tests" / "cpp" / "test_cic_interp.cpp"
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
def test_cic_interpolator_bank_compiles_warning_free(cxx, tmp_path):
    _compile(cxx, tmp_path / "test_cic_interp")


@pytest.mark.gpu
def test_cic_interpolator_bank_matches_the_serial_hogenauer_form_on_gpu(tmp_path):
    exe = _compile("g++", tmp_path / "test_cic_interp")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok")
