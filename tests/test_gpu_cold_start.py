"""The cold start: what a handle created with MMH_LAZY=1 launches, first thing in a fresh process, against what a warmed
handle launches -- the launch description and the bits -- and both against the oracle.

mmh_create warms a handle (csrc/state.hip warm_context): one tile of every kernel MMH_KERNEL_AUTO can pick, which opts each into
more than 64 KiB of LDS, queries each persistent kernel's residency and allocates the null stream's stream-K workspace set; the
opt-ins are remembered per process (csrc/sgemm_tile.hpp opt_in_big_lds).  Every other GPU test runs on a warmed handle in a
process an earlier handle has warmed.  With MMH_LAZY=1 (include/mmult_hip.h; what bench.py's trace run sets and what
warm_context falls back to on a device short of memory) each launch opts in, queries and allocates as it goes, in another order
than the warm-up's: the residency query of a stream-K kernel comes BEHIND its opt-in there and IN FRONT of it in the warm-up.

Each scenario is a fresh child process (tests/cold_start_rows.py holds the rows and runs them in both processes): it checks
MMH_OPT_WARMED == 0 and an empty mmh_last_launch before its first launch, and prints every row's launch string and the SHA-256
of its result.  The parent runs the same rows on a handle it has warmed, compares strings and digests exactly, and its own
result with the oracle's chain (tests/splitk_ref.py for split-K rows, tests/ex_ref.py for epilogues) bit for bit: lazy ==
warmed == reference, no tolerance anywhere.

What the MI355X answered: the occupancy query does not look at the opt-in state, so both orders give one grid, and the
attribute call and the query are accepted on a capturing stream.  A library whose resident_per_cu
answers 1 on a lazy handle fails the "streamk rounds" rows of child A on the launch string and no row on bits.

A child that ends by a signal, an abort or the time limit fails its test with the tail of its output, and the tests behind it
are skipped: nothing more is started on the GPU after such an end."""
import json
import os
import subprocess
import sys

import pytest

import cold_start_rows as rows
from bitcmp import first_difference, same_bits
from built_lib import REPO

pytestmark = pytest.mark.gpu

_CHILD = r"""
import json, os, sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import cold_start_rows
print(json.dumps(cold_start_rows.%s()))
"""
_BAD_END = []   # the child that ended by a signal, an abort or the time limit, if one did


def run_child(scenario):
    """The scenario's JSON line from a fresh process with MMH_LAZY=1 (one child at a time: subprocess.run waits)."""
    if _BAD_END:
        pytest.skip(f"{_BAD_END[0]} ended badly: nothing more is started on the GPU")
    try:
        r = subprocess.run([sys.executable, "-c", _CHILD % scenario, REPO], env=dict(os.environ, MMH_LAZY="1"), capture_output=True,
                           text=True, timeout=300)
    except subprocess.TimeoutExpired as e:
        _BAD_END.append(scenario)
        pytest.fail(f"{scenario} ran into the time limit: {str(e.stdout)[-2000:]} {str(e.stderr)[-2000:]}")
    if r.returncode < 0 or r.returncode in (134, 139, 124, 137):
        _BAD_END.append(scenario)
        pytest.fail(f"{scenario} ended with {r.returncode}: {r.stdout[-2000:]} {r.stderr[-2000:]}")
    assert r.returncode == 0, (scenario, r.stdout[-2000:], r.stderr[-4000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.fixture()
def warmed():
    """The parent's handle: warmed explicitly, so that the comparison holds whatever the environment says."""
    import how_to_optimize_gemm_amd as H
    h = H.MMult(0, "auto")
    h.warm()
    assert h.get_option(H.OPT_WARMED) == 1
    yield h
    timeouts = h.streamk_timeouts()
    h.close()
    assert timeouts == 0


class Differences:
    """Where the lazy handle's rows differ from the warmed handle's: every row is looked at before anything is asserted, the
    bits first -- a launch on another grid keeps them (chained stream-K), so a failure names everything that went wrong."""

    def __init__(self):
        self.bits, self.launches = [], []

    def row(self, child, name, launched, *got):
        if child[name]["sha256"] != rows.digest(*got):
            self.bits.append((name, "lazy:", child[name]["launch"], "warmed:", launched))
        if child[name]["launch"] != launched:
            self.launches.append((name, "lazy:", child[name]["launch"], "warmed:", launched))

    def none(self):
        def lines(found):
            return "\n".join(" | ".join(row) for row in found)
        assert not self.bits, "the lazy handle's bits are not the warmed handle's:\n" + lines(self.bits)
        assert not self.launches, "the lazy handle launched something else than the warmed handle:\n" + lines(self.launches)


def test_forced_kernels_launch_cold_what_they_launch_warm(warmed):
    """Child A: every forced id with symbols of its own through mmh_sgemm on the null stream -- one whole tile, one guarded shape,
    the stream-K forms, the split-K ids -- each the first launch of its kernel symbol in the process (cold_start_rows.forced_rows
    says in which order and why)."""
    import how_to_optimize_gemm_amd as H
    child = run_child("child_forced")
    cus = warmed.device_info()["cu_count"]
    table = rows.forced_rows(cus, H.CHAIN_KERNELS)
    assert child["cus"] == cus and list(child["rows"]) == [r.name for r in table]
    assert {r.kernel for r in table} == set(H.CHAIN_KERNELS) - {"auto"} | set(rows.SPLITK_KERNELS)
    assert {r.kernel for r in table if r.form == "streamk"} == set(rows.STREAMK_KERNELS)
    differences = Differences()
    for row in table:
        launched, got = rows.run_forced(warmed, row)
        assert warmed.streamk_timeouts() == 0, row.name
        rows.check_forced_launch(row, launched)
        differences.row(child["rows"], row.name, launched, got)
        want = rows.forced_reference(row)
        assert same_bits(got, want), (row.name, launched, first_difference(got, want))
    differences.none()


def test_auto_front_ends_launch_cold_what_they_launch_warm(warmed):
    """Child B: MMH_KERNEL_AUTO through the tensor front ends on one lazy handle, each call the first use of its form; then the
    handle is warmed (twice) and repeats its first call; then a handle created warmed runs a stream-K kernel beside it."""
    child = run_child("child_auto")
    cus = warmed.device_info()["cu_count"]
    assert child["cus"] == cus
    steps = rows.auto_steps()
    assert list(child["rows"]) == [name for name, _, _, _ in steps]
    differences = Differences()
    for name, run, reference, planned in steps:
        launched, got = run(warmed, cus)
        assert warmed.streamk_timeouts() == 0, name
        differences.row(child["rows"], name, launched, *got)
        want = reference(cus)
        assert len(got) == len(want), name
        for g, w in zip(got, want):
            assert same_bits(g, w), (name, launched, first_difference(g, w) if g.ndim == 2 else "")
        count = planned(cus)
        # what the host plan says is what both handles launched
        assert rows.carried_count(name, launched) == count == rows.carried_count(name, child["rows"][name]["launch"]), \
            (name, count, launched, child["rows"][name]["launch"])
    first = steps[0][0]
    assert "persistent" in child["rows"][first]["launch"] and "persistent" not in child["rows"][steps[1][0]]["launch"], child["rows"]
    assert "concurrent K parts" in child["rows"][steps[-1][0]]["launch"], child["rows"]
    assert child["repeat"] == child["rows"][first], ("warming changed the lazy handle's first launch", child["repeat"], child["rows"][first])
    beside = [r for r in rows.forced_rows(cus, ["mfma_128x64_dma5"]) if r.form.startswith("streamk")]
    assert len(beside) == 3 and len(child["beside"]) == 6
    for row in beside:
        launched, got = rows.run_forced(warmed, row)
        rows.check_forced_launch(row, launched)
        for who in ("created warmed", "created lazy"):
            differences.row(child["beside"], f"{row.name}, {who}", launched, got)
        want = rows.forced_reference(row)
        assert same_bits(got, want), (row.name, launched, first_difference(got, want))
    differences.none()


def test_a_cold_handle_captures_a_kernels_first_launch(warmed):
    """Child C: a lazy handle whose side stream has its workspace set from mmh_reserve_stream captures a kernel's first launch of
    the process -- a 96 KiB opt-in inside the capture; a stream-K launch with its residency query and LDS share --, replays it
    twice into NaN and runs it eagerly: one result (checked in the child), the warmed handle's and the oracle's bits (here)."""
    child = run_child("child_capture")
    cus = warmed.device_info()["cu_count"]
    table = rows.capture_rows(cus)
    assert child["cus"] == cus and list(child["rows"]) == [r.name for r in table]
    differences = Differences()
    for row in table:
        launched, got = rows.run_forced(warmed, row)
        rows.check_forced_launch(row, launched)
        rows.check_forced_launch(row, child["rows"][row.name]["captured"])
        differences.row(child["rows"], row.name, launched, got)
        want = rows.forced_reference(row)
        assert same_bits(got, want), (row.name, launched, first_difference(got, want))
    differences.none()
