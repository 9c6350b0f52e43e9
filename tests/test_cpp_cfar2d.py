"""The C++ surface of the 2-D CFAR plans (sdsp::cfar2d_plan, include/sdsp/cfar2d.h): a program compiled with g++ and clang++ under the
project's warning flags; on the GPU it sends 3 maps of 16 x 33 cells through cfar2d_plan<float> and <double> -- both edge modes, the
peak rule, both variants, several list capacities -- and compares thresholds, decisions and hit lists bit for bit with direct loops
computed in the program."""
import subprocess

import pytest

from conftest import ROOT

SRC = ROOT / "tests" / "cpp" / "test_cfar2d.cpp"
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
def test_cfar2d_plan_compiles_warning_free(cxx, tmp_path):
    _compile(cxx, tmp_path / "test_cfar2d")


@pytest.mark.gpu
def test_cfar2d_plan_matches_direct_loops_on_gpu(tmp_path):
    exe = _compile("g++", tmp_path / "test_cfar2d")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok")
