#!/usr/bin/env python3
"""Differential fuzz of the int8 linear layers on one GPU: libmmult_hip_q8.so, libmmult_hip_q8o.so, libmmult_hip_q8d.so,
libmmult_hip_q4d.so and q8.QWeight / QWeight4 / QRows / qlinear / qlinear_decode against the numpy contracts (tests/qlinear_ref.py,
qchain_ref.py, qdecode_ref.py, q4_ref.py), bit for bit, on the seeded, stratified case list of tests/q8_fuzz.py: seven forms per
case (the row quantiser alone, the layer on fp32 rows, on quantised rows, with an int8 output, two layers chained in place, the
small-batch layer on both outputs, and the same on 4-bit weights: the packer, both outputs, a caller-made image), guard
bands around every window, the refusals the headers state, and after every launch the library's last_launch text against its own
plan function at the device's CU count.  tests/test_gpu_q8_fuzz.py runs the same runner on cases(64, 2026, cus).
usage: python tools/fuzz_q8.py [cases] [seed]   (cases: a multiple of 8; exit 1: failures, exit 2: a HIP error stopped the run)"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]
import torch  # noqa: E402
import how_to_optimize_gemm_amd as H  # noqa: E402
import q8_fuzz  # noqa: E402

cases = int(sys.argv[1]) if len(sys.argv) > 1 else 64
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
cus = int(torch.cuda.get_device_properties(0).multi_processor_count)
tally, bad = {}, 0
for i, case in enumerate(q8_fuzz.cases(cases, seed, cus)):
    try:
        failures = q8_fuzz.run_case(case, cus, tally)
    except (H.MMultError, RuntimeError) as e:   # a HIP error (the library's MMH_ERR_HIP, or torch's): nothing more runs on this device
        print(f"case {i} (stratum {i % q8_fuzz.STRATA}): stopped by {type(e).__name__}: {e}\n  {case}", flush=True)
        sys.exit(2)
    for f in failures:
        print(f"case {i} (stratum {i % q8_fuzz.STRATA}): {f}\n  {case}")
    bad += len(failures)
print(f"int8 layer fuzz: {cases} cases, {tally.get('forms', 0)} forms run ({tally.get('F7', 0)} of them on 4-bit weights), "
      f"{tally.get('refusals', 0)} refusals checked, {bad} failures")
sys.exit(1 if bad else 0)
