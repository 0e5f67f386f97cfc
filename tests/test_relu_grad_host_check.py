"""tools/host_check/relu_grad_host_check.cpp: the kernels of csrc/relu_grad.hpp compiled as host functions and run thread by
thread under the address and undefined-behaviour sanitizers, on exactly sized buffers, against a scalar loop -- an access
outside a window, a misaligned vector access or a wrong bit shows here, on the CPU, before the kernels run on a device."""
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


@pytest.mark.skipif(_clangxx() is None, reason="no clang++ (the header uses clang's vector types)")
def test_the_kernels_as_host_functions_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "relu_grad_host_check")
    src = os.path.join(REPO, "tools", "host_check", "relu_grad_host_check.cpp")
    subprocess.check_call([_clangxx(), "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I" + os.path.join(REPO, "tools", "host_check"), src, "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "all equal" in run.stdout, run.stdout
    # 8 x 9 shapes and the 4 x 2 at the finish kernel's batch boundaries, x 3 layouts x 7 modes
    assert "emulated %d cases" % ((8 * 9 + 4 * 2) * 3 * 7) in run.stdout, run.stdout
