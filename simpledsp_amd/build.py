"""Build libsdsp_hip.so for gfx950 with hipcc (cross-compiles without a GPU).

Objects go to build/obj (git-ignored); the shared library is written in-tree to
simpledsp_amd/lib/ so that it travels with the source snapshot to the GPU box.
"""
from __future__ import annotations

import hashlib
import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

PKG = Path(__file__).resolve().parent
ROOT = PKG.parent
CSRC = PKG / "csrc"
LIB_DIR = PKG / "lib"
LIB_PATH = LIB_DIR / "libsdsp_hip.so"
OBJ_DIR = ROOT / "build" / "obj"

ARCH = "gfx950"
COMMON = ["-O3", "-std=c++17", "-fPIC", f"--offload-arch={ARCH}", f"-I{ROOT / 'include'}", f"-I{CSRC}",
          "-Wall", "-Wno-unused-function"]
# per-source extra flags.  -fno-slp-vectorize: packing scalar f32 math into v_pk_*_f32 buys nothing on
# CDNA4's SIMD-32 and costs v_mov shuffles + register-pair constraints (measured: fft4096 +1.8 %,
# fft_reg up to +7 %, fft1m +17 % and no scratch, iir -800 v_mov per kernel).  iir.hip keeps the reference's operation order (no FMA contraction) so
# that the f64 kernel reproduces casc_2o_iir.h bit for bit.
SOURCES = {
    "host_math.cpp": ["-x", "hip"],
    "capi.hip": [],
    "fft_tile.hip": [],
    "fft4096.hip": ["-fno-slp-vectorize"],
    "fft1m.hip": ["-fno-slp-vectorize"],  # SLP packing cost 44-76 B/lane of scratch here
    "fft_reg.hip": ["-fno-slp-vectorize"],
    "fft_reg64.hip": ["-fno-slp-vectorize"],
    "fft_big.hip": ["-fno-slp-vectorize"],
    "fft_big64.hip": ["-fno-slp-vectorize"],
    "fft_mix.hip": ["-fno-slp-vectorize"],
    "fft_wave.hip": ["-fno-slp-vectorize"],
    "fft_mid.hip": ["-fno-slp-vectorize"],
    "fft_2pass.hip": ["-fno-slp-vectorize"],
    "fft_cols.hip": ["-fno-slp-vectorize"],
    "iir.hip": ["-ffp-contract=off", "-fno-slp-vectorize"],
    "iir_filtfilt.hip": ["-ffp-contract=off", "-fno-slp-vectorize"],  # iir.hip's recurrence (iir_step.h), bit for bit
    "fir.hip": ["-ffp-contract=off", "-fno-slp-vectorize"],  # f64 taps: multiply then add, like the oracle
    "fir_fft.hip": [],
    "fir_resample.hip": ["-ffp-contract=off", "-fno-slp-vectorize"],  # f64: multiply then add per tap, as fir.hip
    "arb_resample.hip": ["-ffp-contract=off", "-fno-slp-vectorize"],  # f64 taps and a + mu b: multiply then add, never an FMA
    "cic.hip": [],  # integer arithmetic mod 2^W; the one float step is a product with nothing to contract
    "cic_interp.hip": [],  # as cic.hip
    "ddc.hip": ["-ffp-contract=off", "-fno-slp-vectorize"],  # f64 taps and the two complex products: multiply then add, never an FMA
    "duc.hip": ["-ffp-contract=off", "-fno-slp-vectorize"],  # as ddc.hip: f64 taps, the complex products and the band sum never contract
    "beam.hip": ["-ffp-contract=off", "-fno-slp-vectorize"],  # as ddc.hip: f64 taps multiply then add, never an FMA
    "lms.hip": ["-ffp-contract=off", "-fno-slp-vectorize"],  # as ddc.hip; no fast-math either: the NLMS step divides with a correctly rounded `/`
    "rank_filter.hip": [],  # compare-and-select on integer keys only: there is no arithmetic to pin
    "cfar.hip": ["-ffp-contract=off"],  # the I/Q power as stft.hip's; thr = fl(fl(lag + lead) c): a sum then a product, never an FMA
    "cfar2d.hip": ["-ffp-contract=off"],  # as cfar.hip: sums then one product, never an FMA
    "pll.hip": ["-ffp-contract=off", "-fno-slp-vectorize"],  # as ddc.hip: the complex products and the f64 loop filter never contract; no fast-math
    "timing.hip": ["-ffp-contract=off", "-fno-slp-vectorize"],  # as pll.hip: the f64 taps, detector and loop filter never contract; no fast-math
    "viterbi.hip": [],  # integers throughout; the one float step is the product of the F32 quantiser, with nothing to contract
    # GF(256) on integers and table look-ups, no floating point at all.  The plain kernel's per-thread polynomials stay in scratch: turned
    # into registers they cost 256 VGPRs, 114 AGPRs and 1817 spilled SGPRs, one wave per SIMD (profiles/rs_kernel_regs.txt)
    "rs.hip": ["-mllvm", "-disable-promote-alloca-to-vector"],
    "fsync.hip": [],  # bits, shifts and popcounts: no floating point at all
    "ldpc.hip": [],  # integers throughout; the one float step is the product of the F32 quantiser, as in viterbi.hip
    "stft.hip": ["-ffp-contract=off"],  # power = re re + im im: two products and a sum, never an FMA
    "istft.hip": ["-ffp-contract=off"],  # overlap-add: fl(g z) then one addition per frame, never an FMA
    "welch.hip": ["-ffp-contract=off"],  # detrend, window and power: every product and sum rounded on its own, never an FMA
    "csd.hip": ["-ffp-contract=off"],  # cross power: four products, a sum and a difference, each rounded on its own, never an FMA
    "pfb.hip": ["-ffp-contract=off"],  # the fold: fl(x h) then one addition per tap, never an FMA
    "pfb_synth.hip": ["-ffp-contract=off"],  # the unfold: fl(g v) then one addition per frame, never an FMA
    "stream_carry.hip": [],  # the banks' carried state: copies only, no arithmetic to pin
}


def hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and Path(cand).exists():
            return cand
    raise RuntimeError("hipcc not found (need ROCm to build libsdsp_hip.so)")


def source_hash() -> str:
    """sha256 over everything the library is built from: csrc/*, include/**, and this file's flags"""
    h = hashlib.sha256()
    # (everything through the resolved package path: the tree may be reached through a symlink, as /root/repo is on the GPU box)
    files = sorted(CSRC.glob("*")) + sorted((ROOT / "include").rglob("*.h")) + [Path(__file__).resolve()]
    for f in files:
        if f.is_file():
            h.update(f.relative_to(ROOT).as_posix().encode())
            h.update(b"\0")
            h.update(f.read_bytes())
    return h.hexdigest()[:16]


def _dep_files(dfile: Path):
    """prerequisites listed in a compiler-written Makefile fragment (-MMD -MF), or None when it is missing"""
    if not dfile.exists():
        return None
    text = dfile.read_text().replace("\\\n", " ")
    deps = []
    for line in text.splitlines():
        if ":" in line:
            deps += line.split(":", 1)[1].split()
    return [_in_tree(Path(d)) for d in deps]


def _in_tree(dep: Path) -> Path:
    """a prerequisite recorded under another root -- the build directory moved with its tree, or the tree is reached through
    another path than the one the objects were compiled under -- is this tree's file of the same relative name where there is
    one: staleness is about the sources the next build would read, not about where they lay when the object was made"""
    try:
        dep.relative_to(ROOT)
        return dep
    except ValueError:
        pass
    parts = dep.parts
    for anchor in (("simpledsp_amd", "csrc"), ("include",)):
        k = len(anchor)
        for i in range(len(parts) - k - 1, -1, -1):
            if parts[i:i + k] == anchor:
                here = ROOT.joinpath(*parts[i:])
                if here.is_file():
                    return here
                break
    return dep


def _stale(target: Path, deps) -> bool:
    if not target.exists():
        return True
    t = target.stat().st_mtime
    return any((not Path(d).exists()) or Path(d).stat().st_mtime > t for d in deps)


def object_stale(obj: Path, src: Path) -> bool:
    """an object is rebuilt when the compiler's own dependency list for it (every header it included, transitively) has a
    newer file, or when that list does not exist yet; build.py itself (the flags) counts as a prerequisite"""
    deps = _dep_files(obj.with_suffix(".d"))
    if deps is None:
        return True
    return _stale(obj, [src, Path(__file__).resolve(), *deps])


def build_library(force: bool = False, verbose: bool = False) -> Path:
    cc = hipcc()
    OBJ_DIR.mkdir(parents=True, exist_ok=True)
    LIB_DIR.mkdir(parents=True, exist_ok=True)
    digest = source_hash()
    stamp = OBJ_DIR / "source_hash.txt"
    jobs = []
    objs = []
    for src, extra in SOURCES.items():
        obj = OBJ_DIR / (src.rsplit(".", 1)[0] + ".o")
        objs.append(obj)
        flags = list(extra)
        stale = force or object_stale(obj, CSRC / src)
        if src == "host_math.cpp":  # carries the hash: rebuilt whenever any source changed
            flags.append(f'-DSDSP_HIP_SOURCE_HASH="{digest}"')
            stale = stale or not stamp.exists() or stamp.read_text().strip() != digest
        if stale:
            # -MMD -MF: hipcc compiles host and device in one go; the host pass writes the dependency file
            jobs.append([cc, *COMMON, *flags, "-MMD", "-MF", str(obj.with_suffix(".d")), "-c", str(CSRC / src), "-o", str(obj)])

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"{' '.join(cmd)}\n{r.stdout}\n{r.stderr}")
        if verbose and r.stderr.strip():
            print(r.stderr, file=sys.stderr)

    with ThreadPoolExecutor(max_workers=min(4, max(1, len(jobs)))) as ex:
        list(ex.map(run, jobs))
    if force or jobs or _stale(LIB_PATH, objs):
        run([cc, "-shared", "-fPIC", f"--offload-arch={ARCH}", *map(str, objs), "-o", str(LIB_PATH), "-lpthread"])
    stamp.write_text(digest + "\n")
    return LIB_PATH


if __name__ == "__main__":
    print(build_library(force="--force" in sys.argv, verbose=True))
