#!/usr/bin/env python3
"""Differential fuzz of the fp32 tensor front end on one GPU: MMult.matmul, addmm, linear, bmm, baddbmm, batched_linear,
relu_grad_colsum, linear_backward and autograd.linear on views -- row-strided windows, storage offsets, transposed views, single
rows and columns, expanded / gapped / odd batch strides, sizes of 0 and 1 -- carved from NaN-filled storage, against numpy (the
oracle's fused chain, tests/ex_ref.py, tests/relu_grad_ref.py), bit for bit, guard floats included, on the seeded, stratified case
list of tests/front_fuzz.py; on AUTO, the three K2W tiles forced and the tiles with stream-K forced, on torch's current stream
and a side stream; after every launch the library's last_launch text against the addressing model's launch and, on AUTO, the
library's plan functions.  tests/test_gpu_front_fuzz.py runs the same runner on cases(64, 2026, cus).
usage: python tools/fuzz_front.py [cases] [seed]   (cases: a multiple of 8; exit 1: failures, exit 2: a HIP error stopped the run)"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]
import torch  # noqa: E402
import how_to_optimize_gemm_amd as H  # noqa: E402
import front_fuzz  # noqa: E402

cases = int(sys.argv[1]) if len(sys.argv) > 1 else 64
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
tally, bad = {}, 0
with H.MMult(0, "auto") as handle:
    cus = handle.device_info()["cu_count"]
    for case in front_fuzz.cases(cases, seed, cus):
        where = f"case {case.index} (stratum {case.stratum}, {case.family} batch {case.batch} m {case.m} n {case.n} k {case.k} {case.kinds})"
        try:
            failures = front_fuzz.run_case(case, cus, tally, H, handle)
        except (H.MMultError, RuntimeError) as e:   # a HIP error (the library's MMH_ERR_HIP, or torch's): nothing more runs on this device
            print(f"{where}: stopped by {type(e).__name__}: {e}", flush=True)
            sys.exit(2)
        for f in failures:
            print(f"{where}: {f}")
        bad += len(failures)
print(f"fp32 front end fuzz: {cases} cases, {tally.get('forms', 0)} forms run, {tally.get('refusals', 0)} refusals checked, {bad} failures")
sys.exit(1 if bad else 0)
