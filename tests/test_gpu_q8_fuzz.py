"""The int8 layers' differential fuzz on the GPU: tests/q8_fuzz.py's run_case on the seeded list cases(64, 2026, cus), one test per
stratum (eight cases each), and tools/fuzz_q8.py once as a child process on another seed.  What the list reaches and what its
oracle tells apart is held on the CPU by tests/test_q8_fuzz_cases.py; run_case holds every launch's last_launch text to the
library's plan function, so the coverage proved there is the coverage reached here.  The cases of at most 16 rows run the 4-bit
weight too (F7: libmmult_hip_q4d.so through q8.QWeight4 and qlinear_decode)."""
import pytest

import q8_fuzz as F
from gpu_operands import cus_fixture, handle_fixture

pytestmark = pytest.mark.gpu

amm = handle_fixture()        # asked for the device's CU count only
cus = cus_fixture("amm")

N, SEED = 64, 2026
STRATA = ["whole 128 tiles", "ragged small, aligned", "ragged small, unaligned", "around the 128 tile's edges", "decode, aligned",
          "decode, unaligned", "wide rows", "the 256 tile"]


@pytest.mark.parametrize("stratum", range(F.STRATA), ids=lambda s: f"{s}-{STRATA[s].replace(' ', '-').replace(',', '')}")
def test_every_case_of_the_stratum_is_the_contract_in_every_form(stratum, cus):
    cases = F.cases(N, SEED, cus)[stratum::F.STRATA]
    assert len(cases) == N // F.STRATA
    tally, failures = {}, []
    for i, c in enumerate(cases):
        failures += [f"case {F.STRATA * i + stratum}: {f}\n  {c}" for f in F.run_case(c, cus, tally)]
    assert not failures, f"{len(failures)} failures\n" + "\n".join(failures)
    assert tally["forms"] >= 3 * len(cases), tally   # F1, F2 and F4 at the least, in every case
    if stratum in (4, 5):                             # F7: the 4-bit weight's layer on both outputs wherever the split count is valid
        assert tally.get("F7", 0) >= 2 * sum(F.layout(c).splits_ok for c in cases), tally


def test_the_tool_on_another_seed():
    """tools/fuzz_q8.py 16 7 in a child process: exit 0 and its summary line."""
    import os
    import subprocess
    import sys
    from conftest import REPO
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "fuzz_q8.py"), "16", "7"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    last = r.stdout.strip().splitlines()[-1]
    assert last.startswith("int8 layer fuzz: 16 cases, ") and last.endswith(", 0 failures"), last
