"""The memory-queue order K3p's persistent loop counts on, read from the built library's disassembly (no GPU).

igemm_s8_pp_kernel (csrc/igemm_s8_pp.hpp) requests the next tile's prologue -- its LDS-DMA pieces -- in front of the
finished tile's C stores, and the next tile's first two waits are `s_waitcnt vmcnt(4 + STORES)`: "every piece requested in
front of the stores has landed", because returns come back in order.  Nothing in the source forces the compiler to keep
that order; if it ever moved one store above the pieces, or emitted a different number of stores, those waits would let
phase (0, 0) read LDS before its slices are there, and the kernel would return wrong integers without a fault.  This
test holds the whole-tile instantiations (the ones that take the counted waits) to that order.  The expected counts are
read off the kernel's own source."""
import os
import re
import shutil
import struct
import subprocess
import tempfile

import pytest

from built_lib import LIB, REPO, needs_library

SRC = os.path.join(REPO, "how-to-optimize-gemm_amd", "csrc", "igemm_s8_pp.hpp")
OBJDUMP = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-objdump")
pytestmark = [needs_library,
              pytest.mark.skipif(not (os.path.exists(OBJDUMP) or shutil.which("llvm-objdump")), reason="no llvm-objdump")]

INSTRUCTION = re.compile(r"^\s+(?P<text>\S.*?)\s*//\s*(?P<addr>[0-9A-Fa-f]+):(?P<rest>.*)$")
TARGET = re.compile(r"<[^>+]+\+0x(?P<off>[0-9a-f]+)>")


def source_constants():
    """(pieces of a tile's prologue per wave, C stores per wave and whole tile, pieces per phase) from igemm_s8_pp.hpp."""
    src = open(SRC).read()
    tm, tn = map(int, re.search(r"constexpr int BM = 256, BN = 256, TM = (\d+), TN = (\d+);", src).groups())
    request = re.search(r"auto request = \[&\].*?\n  \};", src, re.S).group(0)
    per_request = int(re.search(r"for \(int j = 0; j < (\d+); \+\+j\)", request).group(1))   # pieces of one region per wave
    prologue = re.search(r"auto request_prologue = \[&\].*?\n  \};", src, re.S).group(0)
    regions = len(re.findall(r"\brequest\(t, ", prologue))
    phase = re.search(r"if constexpr \(S == 0\) \{(.*?)\}", src, re.S).group(1)          # the regions one phase requests
    return regions * per_request, tm * tn, len(re.findall(r"\brequest\(cur, ", phase)) * per_request


def _code_object_with(blob, mangled):
    import kernel_resources as K
    for off in K.code_objects(blob):
        e_shoff = struct.unpack_from("<Q", blob, off + 0x28)[0]
        e_shentsize, e_shnum = struct.unpack_from("<HH", blob, off + 0x3A)
        elf = blob[off:off + e_shoff + e_shentsize * e_shnum]
        if mangled.encode() in elf:
            return elf
    raise AssertionError(f"{mangled} is in no code object of libmmult_hip.so")


def disassemble(mfma_k):
    """[(offset from the kernel's entry, instruction text, the encoding and branch target)] of
    igemm_s8_pp_kernel<false,false,MFMA_K>."""
    mangled = f"_ZN3mmh18igemm_s8_pp_kernelILb0ELb0ELi{mfma_k}EEEviiiPKaiS2_iPiiiiiPKf"
    elf = _code_object_with(open(LIB, "rb").read(), mangled)
    exe = OBJDUMP if os.path.exists(OBJDUMP) else shutil.which("llvm-objdump")
    with tempfile.NamedTemporaryFile(suffix=".co") as f:
        f.write(elf)
        f.flush()
        out = subprocess.run([exe, "-d", f"--disassemble-symbols={mangled}", f.name], capture_output=True, text=True,
                             check=True).stdout
    entry = re.search(r"^([0-9a-f]+) <" + re.escape(mangled) + ">:", out, re.M)
    assert entry, out[:2000]
    base = int(entry.group(1), 16)
    ins = []
    for line in out.splitlines():
        m = INSTRUCTION.match(line)
        if m:
            ins.append((int(m["addr"], 16) - base, m["text"], m["rest"]))
    assert len(ins) > 500, len(ins)
    return ins


def _is_piece(text):
    return re.match(r"buffer_load_dword\S*\s.*\blds$", text) is not None


def _is_vmem_store(text):
    return re.match(r"(global|buffer|flat)_store_", text) is not None


@pytest.mark.parametrize("mfma_k", [64, 32])
def test_the_next_tiles_pieces_precede_the_stores_its_first_waits_count(mfma_k):
    pieces, stores, per_phase = source_constants()
    assert (pieces, stores, per_phase) == (10, 32, 4), "the kernel's constants changed: re-read the counted waits"
    wait = f"s_waitcnt vmcnt({per_phase + stores})"
    ins = disassemble(mfma_k)
    texts = [t for _, t, _ in ins]
    at = [i for i, t in enumerate(texts) if _is_piece(t)]
    # the tile's end: the last `pieces` LDS-DMA requests of the kernel are the next tile's prologue ...
    prologue = at[-pieces:]
    assert len(prologue) == pieces
    drain = max(i for i, t in enumerate(texts[:prologue[0]]) if re.fullmatch(r"s_waitcnt vmcnt\(0\)", t))
    between = texts[drain:prologue[-1]]
    assert not any(_is_vmem_store(t) for t in between), "a C store was issued in front of the next tile's prologue"
    assert sum(_is_piece(t) for t in between) == pieces - 1, "the prologue is split by another LDS-DMA request"
    # ... behind them exactly `stores` C stores of 16 bytes each, and no further request of any kind
    tail = texts[prologue[-1] + 1:]
    assert sum(t.startswith("global_store_dwordx4 ") for t in tail) == stores, [t for t in tail if _is_vmem_store(t)]
    assert not any(_is_vmem_store(t) and not t.startswith("global_store_dwordx4 ") for t in tail)
    assert not any(_is_piece(t) for t in tail), "an LDS-DMA request behind the C stores"
    # the next tile's first waits -- the loop head and phase (0, 0) -- count past exactly those stores ...
    waits = [i for i, t in enumerate(texts) if t.startswith(wait + " ") or t == wait]
    assert len(waits) == 2, [texts[i] for i in waits]
    assert texts[waits[0]] == wait and texts[waits[1]] == wait + " lgkmcnt(0)", [texts[i] for i in waits]
    assert all(w < prologue[0] for w in waits)
    # ... and run after them: the tile loop's back edge, behind the last store, jumps to the loop head in front of both
    last_store = max(i for i, t in enumerate(texts) if t.startswith("global_store_dwordx4 "))
    back = [int(m["off"], 16) for _, t, rest in ins[last_store:] if t.startswith("s_") and (m := TARGET.search(rest))]
    head = ins[waits[0]][0]
    assert any(off <= head for off in back), "no branch from behind the stores back to the counted waits"
