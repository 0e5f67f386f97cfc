"""The fp32 tensor front end's differential fuzz on the GPU: tests/front_fuzz.py's run_case on the seeded list
cases(64, 2026, cus), one test per stratum (eight cases each), and tools/fuzz_front.py once as a child process on another seed.
What the list reaches and which wrong front ends its expectations tell apart is held on the CPU by
tests/test_front_fuzz_cases.py; run_case holds every launch's last_launch text to the addressing model's launch and, on AUTO, to
the library's plan functions at the device's CU count."""
import pytest

import front_fuzz as F
from gpu_operands import cus_fixture, handle_fixture

pytestmark = pytest.mark.gpu

amm = handle_fixture(check_timeouts=True)
cus = cus_fixture("amm")

N, SEED = 64, 2026


@pytest.mark.parametrize("stratum", range(F.STRATA), ids=lambda s: f"{s}-{F.STRATUM_NAMES[s].replace(' ', '-')}")
def test_every_case_of_the_stratum_is_the_numpy_contract_in_every_form(stratum, amm, cus):
    import how_to_optimize_gemm_amd as H
    cases = F.cases(N, SEED, cus)[stratum::F.STRATA]
    assert len(cases) == N // F.STRATA
    tally, failures = {}, []
    for c in cases:
        failures += [f"case {c.index}: {f}\n  {describe(c)}" for f in F.run_case(c, cus, tally, H, amm)]
    assert not failures, f"{len(failures)} failures\n" + "\n".join(failures)
    if F.STRATUM_NAMES[stratum] == "refusals":
        assert tally.get("refusals", 0) >= 3 * len(cases) and "forms" not in tally, tally
    else:
        assert tally["forms"] >= 9 * len(cases), tally      # the 2-D family's nine forms at the least, in every case


def describe(c):
    return f"{c.family} batch {c.batch} m {c.m} n {c.n} k {c.k} alpha, beta {c.ab} relu {c.relu} bias {c.bias} side stream {c.side_stream} " \
           f"{c.kinds} {c.refusal or ''}"


def test_the_tool_on_another_seed():
    """tools/fuzz_front.py 16 7 in a child process: exit 0 and its summary line."""
    import os
    import subprocess
    import sys
    from built_lib import REPO
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "fuzz_front.py"), "16", "7"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    last = r.stdout.strip().splitlines()[-1]
    assert last.startswith("fp32 front end fuzz: 16 cases, ") and last.endswith(", 0 failures"), last
