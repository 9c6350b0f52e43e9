"""The C++ surface of the column FFT plans (sdsp::fft_cols_plan, include/sdsp/fft_cols.h): a program compiled with g++ and clang++
under the project's warning flags; on the GPU it sends a 3 x 64 x 33 cube through fft_cols_plan<float> and <double> -- forward in
place, reverse, and a windowed, shifted power plan -- and compares with a direct double DFT computed in the program."""
import subprocess

import pytest

from conftest import ROOT

SRC = ROOT / "tests" / "cpp" / "test_fft_cols.cpp"
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
def test_fft_cols_plan_compiles_warning_free(cxx, tmp_path):
    _compile(cxx, tmp_path / "test_fft_cols")


@pytest.mark.gpu
def test_fft_cols_plan_matches_a_direct_dft_on_gpu(tmp_path):
    exe = _compile("g++", tmp_path / "test_fft_cols")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok")
