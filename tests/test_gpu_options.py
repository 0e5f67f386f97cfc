"""Every handle option of include/mmult_hip.h read back after it is set (mmh_set_option / mmh_get_option, csrc/abi.hip): the
default, every accepted boundary value and what get then returns, the first value outside each bound -- refused with
MMH_ERR_INVALID_ARG, the option unchanged --, and ids that are no option, in both directions.  The expectations are the
product library's; the tools build accepts more (tests/test_tools_build.py).

The handle is the test's own; nothing is launched on it (fault injection is on for two calls), and every option is back at
its default before it closes."""
import ctypes

import pytest

pytestmark = pytest.mark.gpu

INT_MIN, INT_MAX = -(1 << 31), (1 << 31) - 1


@pytest.fixture()
def opts(monkeypatch):
    """set(option, value) -> status and get(option) -> (status, value) on a fresh handle, plus the module."""
    import how_to_optimize_gemm_amd as H
    monkeypatch.delenv("MMH_NO_SK_ORDER", raising=False)   # (read at mmh_create: it would change MMH_OPT_STREAMK_ORDER's default)
    monkeypatch.delenv("MMH_LAZY", raising=False)          # (read at mmh_create: MMH_OPT_WARMED would read 0)
    assert H.lib().mmh_is_ab_build() == 0
    mm = H.MMult(0, "auto")

    def set_(option, value):
        return H.lib().mmh_set_option(mm._h, option, value)

    def get(option):
        v = ctypes.c_int(-12345)
        return H.lib().mmh_get_option(mm._h, option, ctypes.byref(v)), v.value

    yield H, set_, get
    timeouts = mm.streamk_timeouts()
    mm.close()
    assert timeouts == 0


def refused(H, set_, get, option, value):
    """`value` is refused and the option reads as before."""
    before = get(option)
    assert before[0] == H.OK, option
    assert set_(option, value) == H.ERR_INVALID_ARG, (option, value)
    assert get(option) == before, (option, value)


def test_every_option_reads_back_what_set_made_of_the_value(opts):
    H, set_, get = opts
    # option: (lowest accepted, highest accepted, default) -- get returns the value that was set
    ranges = {H.OPT_STREAMK: (0, 2, 1), H.OPT_SPLITK: (0, 16, 0), H.OPT_HOST_PANELS: (-1, 16, -1), H.OPT_PERSIST: (0, 1, 0),
              H.OPT_STREAMK_SPIN_LIMIT: (1, INT_MAX, 65536),
              H.OPT_RIM: (0, 0, 0), H.OPT_RIM5: (0, 0, 0)}   # (the product accepts "off" only)
    # option: default -- any value is accepted, get returns 0 for 0 and 1 for everything else
    switches = {H.OPT_STREAMK_ORDER: 1, H.OPT_STREAMK_CHAIN: 1, H.OPT_FAULT_INJECT: 0}
    try:
        for option, (lo, hi, default) in ranges.items():
            assert get(option) == (H.OK, default), option
            for value in sorted({lo, hi, default}):
                assert set_(option, value) == H.OK, (option, value)
                assert get(option) == (H.OK, value), (option, value)
                refused(H, set_, get, option, lo - 1)
                if hi < INT_MAX:
                    refused(H, set_, get, option, hi + 1)
            assert set_(option, default) == H.OK
        for option, default in switches.items():
            assert get(option) == (H.OK, default), option
            for value, reads in ((1, 1), (0, 0), (3, 1), (7, 1), (-1, 1), (INT_MIN, 1), (INT_MAX, 1), (0, 0)):
                assert set_(option, value) == H.OK, (option, value)
                assert get(option) == (H.OK, reads), (option, value)
                if option == H.OPT_FAULT_INJECT:   # never on for longer than it takes to read it back
                    assert set_(option, 0) == H.OK and get(option) == (H.OK, 0)
            assert set_(option, default) == H.OK
        # MMH_OPT_DMA_EDGE: 0, 1, 2; every other value reads as the nearest of them that it switches on
        assert get(H.OPT_DMA_EDGE) == (H.OK, 2)
        for value, reads in ((0, 0), (1, 1), (2, 2), (3, 2), (5, 2), (INT_MAX, 2), (-1, 1), (INT_MIN, 1)):
            assert set_(H.OPT_DMA_EDGE, value) == H.OK, value
            assert get(H.OPT_DMA_EDGE) == (H.OK, reads), value
        assert set_(H.OPT_DMA_EDGE, 2) == H.OK
        # MMH_OPT_IGEMM_MODE: 0 .. 9 without the tools build's 1, 3 and 4
        assert get(H.OPT_IGEMM_MODE) == (H.OK, 0)
        for value in range(-2, 16):
            if value in (0, 2, 5, 6, 7, 8, 9):
                assert set_(H.OPT_IGEMM_MODE, value) == H.OK, value
                assert get(H.OPT_IGEMM_MODE) == (H.OK, value), value
            else:
                refused(H, set_, get, H.OPT_IGEMM_MODE, value)
        assert set_(H.OPT_IGEMM_MODE, 0) == H.OK
        # the two counters: 0 on a handle that is in order; writing 0 clears, nothing else can be written
        assert get(H.OPT_STREAMK_TIMEOUTS) == (H.OK, 0)
        status, delegations = get(H.OPT_STREAMK_DELEGATIONS)   # (the warm-up's launches may have counted)
        assert status == H.OK and delegations >= 0
        for option in (H.OPT_STREAMK_TIMEOUTS, H.OPT_STREAMK_DELEGATIONS):
            assert set_(option, 0) == H.OK, option
            assert get(option) == (H.OK, 0), option
            for value in (1, -1, INT_MAX, INT_MIN):
                refused(H, set_, get, option, value)
        # MMH_OPT_RETIRED_BUFFERS: read-only -- 0 on a handle that has captured nothing; no value can be written, 0 included
        assert get(H.OPT_RETIRED_BUFFERS) == (H.OK, 0)
        for value in (0, 1, -1, INT_MAX, INT_MIN):
            refused(H, set_, get, H.OPT_RETIRED_BUFFERS, value)
        # MMH_OPT_WARMED: read-only -- 1 on a handle mmh_create has warmed (0 only under MMH_LAZY=1, tests/test_gpu_cold_start.py)
        assert get(H.OPT_WARMED) == (H.OK, 1)
        for value in (0, 1, -1, INT_MAX, INT_MIN):
            refused(H, set_, get, H.OPT_WARMED, value)
        # ids that are no option of the product: below and above the public ones, and the tools build's 100 .. 108
        for option in [0, -1, 17, 18, 99, INT_MAX, INT_MIN] + list(range(100, 110)):
            for value in (0, 1):
                assert set_(option, value) == H.ERR_INVALID_ARG, (option, value)
            assert get(option) == (H.ERR_INVALID_ARG, -12345), option
    finally:
        for option, (_, _, default) in ranges.items():
            set_(option, default)
        for option, default in switches.items():
            set_(option, default)
        set_(H.OPT_DMA_EDGE, 2)
        set_(H.OPT_IGEMM_MODE, 0)
    defaults = {**{o: r[2] for o, r in ranges.items()}, **switches, H.OPT_DMA_EDGE: 2, H.OPT_IGEMM_MODE: 0,
                H.OPT_STREAMK_TIMEOUTS: 0, H.OPT_STREAMK_DELEGATIONS: 0, H.OPT_RETIRED_BUFFERS: 0, H.OPT_WARMED: 1}
    assert sorted(defaults) == list(range(1, 17))   # every public MMH_OPT_* was covered
    for option, default in defaults.items():
        assert get(option) == (H.OK, default), option
