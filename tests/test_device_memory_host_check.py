"""tools/host_check/device_memory_host_check.cpp: the product's own memory code -- csrc/device_memory.hpp and csrc/state.hip --
compiled as host code against a stand-in for the HIP runtime and run under the address and undefined-behaviour sanitizers:
growth, refusal under capture, retirement, eviction of stream sets and tables, failed allocations and destruction, on the CPU.
The stand-in counts live allocations itself: that count, not the sanitizer's leak checker, is the leak check."""
import os
import shutil
import subprocess

import pytest

from built_lib import REPO


def _clangxx():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    roots = [os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), os.environ.get("ROCM_PATH", "/opt/rocm"), "/opt/rocm"]
    for cand in [os.path.join(r, "llvm", "bin", "clang++") for r in roots] + [shutil.which("clang++")]:
        if cand and os.path.exists(cand):
            return cand
    return None


@pytest.mark.skipif(_clangxx() is None, reason="no clang++")
def test_the_memory_manager_as_host_code_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "device_memory_host_check")
    check = os.path.join(REPO, "tools", "host_check")
    subprocess.check_call([_clangxx(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I" + os.path.join(check, "device_stub"),
                           os.path.join(check, "device_memory_host_check.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    last = run.stdout.strip().splitlines()[-1]
    assert last.startswith("device memory host check: 9 scenarios passed"), run.stdout
    assert last.endswith("0 allocations left"), run.stdout
