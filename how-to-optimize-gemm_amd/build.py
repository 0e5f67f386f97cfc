"""Build recipe for libmmult_hip.so (hipcc, gfx950 only) and the C++ harness.

`python -m how_to_optimize_gemm_amd.build` or __graft_entry__.build() runs it.
The library is built IN-TREE next to this file so that it travels with the
repository snapshot to the GPU box; nothing is installed into site-packages.
"""
from __future__ import annotations

import os
import shutil
import subprocess

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(PKG_DIR)
CSRC = os.path.join(PKG_DIR, "csrc")
LIB = os.path.join(PKG_DIR, "libmmult_hip.so")
AB_LIB = os.path.join(PKG_DIR, "libmmult_hip_ab.so")   # tools-only build: A/B variants + timing-only ablations
CSRC_Q8 = os.path.join(PKG_DIR, "csrc_q8")
Q8_LIB = os.path.join(PKG_DIR, "libmmult_hip_q8.so")   # the second product library: the int8 linear layer (include/mmult_hip_q8.h)
CSRC_Q8O = os.path.join(PKG_DIR, "csrc_q8o")
Q8O_LIB = os.path.join(PKG_DIR, "libmmult_hip_q8o.so")   # the third: the int8 layer with an int8 output (include/mmult_hip_q8o.h)
CSRC_Q8D = os.path.join(PKG_DIR, "csrc_q8d")
Q8D_LIB = os.path.join(PKG_DIR, "libmmult_hip_q8d.so")   # the fourth: the int8 layer for 1 - 16 rows, split-K (include/mmult_hip_q8d.h)
CSRC_Q4D = os.path.join(PKG_DIR, "csrc_q4d")
Q4D_LIB = os.path.join(PKG_DIR, "libmmult_hip_q4d.so")   # the fifth: the 1 - 16 row layer on packed 4-bit weights (include/mmult_hip_q4d.h)
CSRC_Q4G = os.path.join(PKG_DIR, "csrc_q4g")
Q4G_LIB = os.path.join(PKG_DIR, "libmmult_hip_q4g.so")   # the sixth: the 4-bit layer with one scale per group of 128 (include/mmult_hip_q4g.h)
HARNESS = os.path.join(PKG_DIR, "harness")
ARCH = "gfx950"


def hipcc() -> str:
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(exe):
        raise RuntimeError("hipcc not found: the MI355X backend cannot be built")
    return exe


def _stale(target: str, srcs: list[str]) -> bool:
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(s) > t for s in srcs)


def library_sources() -> list[str]:
    out = [os.path.join(REPO, "include", "mmult_hip.h")]
    for f in sorted(os.listdir(CSRC)):
        if f.endswith((".hip", ".hpp", ".inc", ".map")):
            out.append(os.path.join(CSRC, f))
    return out


AB_SRC = os.path.join(REPO, "tools", "ab")   # tile families that were built, measured and lost: tools build only


def translation_units(ab: bool = False) -> list[str]:
    tus = sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hip"))
    if ab and os.path.isdir(AB_SRC):
        tus += sorted(os.path.join(AB_SRC, f) for f in os.listdir(AB_SRC) if f.endswith(".hip"))
    return tus


def _headers(*dirs: str, c_headers: tuple = ()) -> list[str]:
    """What makes an object stale besides its .hip: csrc/'s headers and the first C header, the named C headers of include/,
    and every .hpp of `dirs`."""
    out = [s for s in library_sources() if s.endswith((".hpp", ".h", ".inc"))]
    out += [os.path.join(REPO, "include", h) for h in c_headers]
    for d in dirs:
        out += [os.path.join(d, f) for f in sorted(os.listdir(d)) if f.endswith(".hpp")]
    return out


def _hip_sources(d: str) -> list[str]:
    return sorted(os.path.join(d, f) for f in os.listdir(d) if f.endswith(".hip"))


def _build_shared(target: str, tus: list[str], includes: list[str], headers: list[str], objdir: str, version_script: str,
                  extra: tuple = (), link_flags: tuple = (), force: bool = False, verbose: bool = False) -> str:
    """The one recipe of every library: hipcc -c each translation unit of `tus` with -I `includes` in that order, then `extra`
    (defines, and what goes with them), at most 16 at a time (the kernel-heavy ones take a minute each), then link the objects
    into `target` with `link_flags` and the version script.  Objects live under build/<objdir>/ (git-ignored) and are reused while
    neither their .hip nor any of `headers` has changed."""
    from concurrent.futures import ThreadPoolExecutor
    odir = os.path.join(PKG_DIR, "build", objdir)
    os.makedirs(odir, exist_ok=True)
    flags = [f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-result"] + ["-I" + d for d in includes] + list(extra)
    objs = [os.path.join(odir, os.path.basename(tu)[:-4] + ".o") for tu in tus]
    jobs = [[hipcc()] + flags + ["-c", tu, "-o", obj] for tu, obj in zip(tus, objs) if force or _stale(obj, [tu] + headers)]
    def run(cmd):
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
    if jobs:
        with ThreadPoolExecutor(max_workers=min(len(jobs), os.cpu_count() or 4, 16)) as pool:
            list(pool.map(run, jobs))
    if force or jobs or _stale(target, objs + [version_script]):
        run([hipcc(), f"--offload-arch={ARCH}", "-shared", "-fPIC"] + objs + ["-o", target] + list(link_flags) + ["-Wl,--version-script=" + version_script])
    return target


def _build_product(target: str, defines: list[str], objdir: str, force: bool, verbose: bool) -> str:
    """csrc/*.hip with `defines` -> `target`; -DMMH_AB_BUILD adds tools/ab/'s translation units, headers and -I."""
    ab = "-DMMH_AB_BUILD" in defines
    headers = _headers()
    if ab and os.path.isdir(AB_SRC):
        headers += [os.path.join(AB_SRC, f) for f in sorted(os.listdir(AB_SRC)) if f.endswith((".hpp", ".inc"))]
    return _build_shared(target, translation_units(ab), [CSRC], headers, objdir, os.path.join(CSRC, "exports.map"),
                         defines + (["-I" + AB_SRC] if ab else []), ["-ldl"], force, verbose)


def build_library(force: bool = False, verbose: bool = False) -> str:
    """hipcc --offload-arch=gfx950 -> how-to-optimize-gemm_amd/libmmult_hip.so"""
    return _build_product(LIB, [], "product", force, verbose)


def build_q8_library(force: bool = False, verbose: bool = False) -> str:
    """csrc_q8/*.hip -> how-to-optimize-gemm_amd/libmmult_hip_q8.so, with the product library's flags (-I csrc_q8 -I csrc: its
    kernels sit on csrc/'s int8 tile and quantisation rules).  Objects under build/q8/; an object is stale when its .hip, a header
    of csrc_q8/ or of csrc/, or either C header has changed."""
    return _build_shared(Q8_LIB, _hip_sources(CSRC_Q8), [CSRC_Q8, CSRC], _headers(CSRC_Q8, c_headers=("mmult_hip_q8.h",)), "q8",
                         os.path.join(CSRC_Q8, "exports_q8.map"), force=force, verbose=verbose)


def build_q8o_library(force: bool = False, verbose: bool = False) -> str:
    """csrc_q8o/*.hip -> how-to-optimize-gemm_amd/libmmult_hip_q8o.so: the q8 library's recipe with -I csrc_q8o in front (its host
    side shares csrc_q8/q8_host.hpp).  Objects under build/q8o/; csrc_q8o/'s headers and mmult_hip_q8o.h make them stale too."""
    return _build_shared(Q8O_LIB, _hip_sources(CSRC_Q8O), [CSRC_Q8O, CSRC_Q8, CSRC],
                         _headers(CSRC_Q8, CSRC_Q8O, c_headers=("mmult_hip_q8.h", "mmult_hip_q8o.h")), "q8o",
                         os.path.join(CSRC_Q8O, "exports_q8o.map"), force=force, verbose=verbose)


def build_q8d_library(force: bool = False, verbose: bool = False) -> str:
    """csrc_q8d/*.hip -> how-to-optimize-gemm_amd/libmmult_hip_q8d.so: the q8o library's recipe with -I csrc_q8d in front (its
    kernels use csrc/'s LDS-DMA loader, plan rules and quantisation rules).  Objects under build/q8d/; csrc_q8d/'s headers and
    mmult_hip_q8d.h make them stale too."""
    return _build_shared(Q8D_LIB, _hip_sources(CSRC_Q8D), [CSRC_Q8D, CSRC_Q8O, CSRC_Q8, CSRC],
                         _headers(CSRC_Q8, CSRC_Q8O, CSRC_Q8D, c_headers=("mmult_hip_q8.h", "mmult_hip_q8o.h", "mmult_hip_q8d.h")), "q8d",
                         os.path.join(CSRC_Q8D, "exports_q8d.map"), force=force, verbose=verbose)


def build_q4d_library(force: bool = False, verbose: bool = False) -> str:
    """csrc_q4d/*.hip -> how-to-optimize-gemm_amd/libmmult_hip_q4d.so: the q8d library's recipe with -I csrc_q4d in front (its
    partial kernel sits on csrc_q8d/'s ring geometry and instantiates its finish kernel).  Objects under build/q4d/; csrc_q4d/'s
    headers and mmult_hip_q4d.h make them stale too."""
    return _build_shared(Q4D_LIB, _hip_sources(CSRC_Q4D), [CSRC_Q4D, CSRC_Q8D, CSRC_Q8O, CSRC_Q8, CSRC],
                         _headers(CSRC_Q8, CSRC_Q8O, CSRC_Q8D, CSRC_Q4D,
                                  c_headers=("mmult_hip_q8.h", "mmult_hip_q8o.h", "mmult_hip_q8d.h", "mmult_hip_q4d.h")), "q4d",
                         os.path.join(CSRC_Q4D, "exports_q4d.map"), force=force, verbose=verbose)


def build_q4g_library(force: bool = False, verbose: bool = False) -> str:
    """csrc_q4g/*.hip -> how-to-optimize-gemm_amd/libmmult_hip_q4g.so: the q4d library's recipe with -I csrc_q4g in front (its
    kernels sit on csrc_q8d/'s ring geometry and csrc_q4d/'s quantisation rules and plan geometry).  Objects under build/q4g/;
    csrc_q4g/'s headers and mmult_hip_q4g.h make them stale too."""
    return _build_shared(Q4G_LIB, _hip_sources(CSRC_Q4G), [CSRC_Q4G, CSRC_Q4D, CSRC_Q8D, CSRC_Q8O, CSRC_Q8, CSRC],
                         _headers(CSRC_Q8, CSRC_Q8O, CSRC_Q8D, CSRC_Q4D, CSRC_Q4G,
                                  c_headers=("mmult_hip_q8.h", "mmult_hip_q8o.h", "mmult_hip_q8d.h", "mmult_hip_q4d.h", "mmult_hip_q4g.h")),
                         "q4g", os.path.join(CSRC_Q4G, "exports_q4g.map"), force=force, verbose=verbose)


def build_timeline_library(force: bool = False) -> str:
    """-DMMH_AB_BUILD -DMMH_DMA_TIMELINE -> libmmult_hip_tl.so: the A/B library whose plain LDS-DMA kernels
    also write per-workgroup wall-clock stamps (tools/dma_timeline.py only; the stamps perturb the
    schedule of the big tiles, so no other tool measures with this build)."""
    return _build_product(os.path.join(PKG_DIR, "libmmult_hip_tl.so"), ["-DMMH_AB_BUILD", "-DMMH_DMA_TIMELINE"], "timeline",
                         force, False)


def build_ab_library(force: bool = False, verbose: bool = False) -> str:
    """The same sources with -DMMH_AB_BUILD -> libmmult_hip_ab.so: the product kernels PLUS the
    scheduling A/B variants and the timing-only ablation builds (wrong results).  Loaded by
    tools/ab_bench.py and tools/misc_bench.py only; never by the package, the harness or the tests
    of the product path."""
    return _build_product(AB_LIB, ["-DMMH_AB_BUILD"], "ab", force, verbose)


def build_harness(force: bool = False) -> str:
    """The C++ host side (test_MMult.x and friends) via its makefile."""
    exe = os.path.join(HARNESS, "test_MMult.x")
    args = ["make", "-s", "-C", HARNESS]
    if force:
        subprocess.check_call(args + ["clean"])
    subprocess.check_call(args + ["all"])
    return exe


def build_all(force: bool = False) -> None:
    build_library(force)
    build_q8_library(force)
    build_q8o_library(force)
    build_q8d_library(force)
    build_q4d_library(force)
    build_q4g_library(force)
    if os.path.isdir(HARNESS):
        build_harness(force)


if __name__ == "__main__":
    build_all(force=True)
    print(LIB)
