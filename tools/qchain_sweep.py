#!/usr/bin/env python3
"""qchain_sweep.py -- a two-layer ReLU MLP in int8, rows x 4096 -> 11008 -> 4096, three ways:
  chain     q8.quantize(x), then q8.qlinear(.., out_scale=s) (int8 -> int8, libmmult_hip_q8o.so), then q8.qlinear (int8 -> fp32):
            three launches, the hidden activation crosses memory once, as bytes
  2 qlinear q8.qlinear twice (what there was before): four launches, the hidden activation written as fp32 and read back by
            the second layer's row quantiser
  2 linear  MMult.linear twice, in fp32
and per layer shape the int8-output GEMM alone beside the fp32-output GEMM, both from rows that are quantised already.
Every call is issued from Python between one pair of events per pass; every figure is the median of `--passes` interleaved
passes after a warm-up (tools/qlinear_sweep.py's protocol), and the spread (max - min) of the two-qlinear baseline's own passes
is the yardstick: the chain is "ahead" only where it wins by more than that.  Writes profiles/qchain_sweep.md.

    python tools/qchain_sweep.py [--passes 5] [--reps 20] [--out profiles/qchain_sweep.md]"""
import argparse
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402
import how_to_optimize_gemm_amd as H  # noqa: E402
from how_to_optimize_gemm_amd import q8  # noqa: E402

ROWS = (16, 512, 4096)
D_IN, D_HID, D_OUT = 4096, 11008, 4096


def events(step, reps, warm=0):
    for _ in range(warm):
        step()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        step()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / reps


def passes_of(calls, passes, reps):
    """{name: [ms per pass]} of `passes` interleaved passes over calls = {name: step}."""
    for step in calls.values():
        events(step, 3, 3)
    ms = {name: [] for name in calls}
    for _ in range(passes):
        for name, step in calls.items():
            ms[name].append(events(step, reps))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "qchain_sweep.md"))
    args = ap.parse_args()
    mm = H.MMult(0, "auto")
    w1 = torch.randn((D_HID, D_IN), device="cuda") / D_IN ** 0.5
    w2 = torch.randn((D_OUT, D_HID), device="cuda") / D_HID ** 0.5
    b1, b2 = torch.randn(D_HID, device="cuda") * 0.1, torch.randn(D_OUT, device="cuda") * 0.1
    qw1, qw2 = q8.QWeight(w1), q8.QWeight(w2)
    table = []
    for rows in ROWS:
        x = torch.randn((rows, D_IN), device="cuda")
        mlp = q8.QMLP([qw1, qw2], [b1, b2])
        mlp.calibrate(x)
        so, inv = mlp._vectors[0]
        hf, yf, y2, yl = (torch.empty((rows, n), device="cuda") for n in (D_HID, D_OUT, D_OUT, D_OUT))
        hl = torch.empty((rows, D_HID), device="cuda")
        xq = q8.quantize(x)
        hq_buf = torch.empty((rows, D_HID), dtype=torch.int8, device="cuda")
        hq = q8._linear_s8o("sweep", xq, qw1, b1, "relu", so, inv, hq_buf)

        def two_qlinear():
            q8.qlinear(x, qw1, b1, "relu", out=hf)
            q8.qlinear(hf, qw2, b2, out=y2)

        def two_linear():
            mm.linear(x, w1, b1, activation="relu", out=hl)
            mm.linear(hl, w2, b2, out=yl)

        calls = {
            "chain": lambda: mlp(x),
            "2 qlinear": two_qlinear,
            "2 linear": two_linear,
            "L1 s8->s8": lambda: q8._linear_s8o("sweep", xq, qw1, b1, "relu", so, inv, hq_buf),
            "L1 s8->f32": lambda: q8.qlinear(xq, qw1, b1, "relu", out=hf),
            "L2 s8->s8": lambda: q8._linear_s8o("sweep", hq, qw2, b2, None, so, inv, hq_buf[:, :D_OUT]),
            "L2 s8->f32": lambda: q8.qlinear(hq, qw2, b2, out=yf),
        }
        ms = passes_of(calls, args.passes, args.reps)
        # what ran, and that the chain and the baseline agree to within the hidden layer's quantisation
        calls["L1 s8->s8"]()
        launch1 = q8.last_launch_q8o()
        calls["L2 s8->f32"]()
        launch2 = q8.last_launch()
        yc = mlp(x)
        two_qlinear()
        torch.cuda.synchronize()
        rel = float((yc - y2).abs().max() / y2.abs().max())
        table.append((rows, ms, launch1, launch2, rel))
        print(rows, " ".join(f"{k} {statistics.median(v) * 1e3:.1f}us" for k, v in ms.items()), f"max rel diff {rel:.3g}", flush=True)
        del x, mlp, hf, yf, y2, yl, hl, xq, hq_buf, hq
    dev = "MI355X" if "gfx950" in torch.cuda.get_device_properties(0).gcnArchName else torch.cuda.get_device_properties(0).name
    with open(args.out, "w") as fo:
        fo.write("# A two-layer int8 MLP as a chain of int8-to-int8 layers, beside two qlinear calls and fp32\n\n")
        fo.write(f"`python tools/qchain_sweep.py --passes {args.passes} --reps {args.reps}` on one {dev}: rows x {D_IN} -> {D_HID} (bias, ReLU) "
                 f"-> {D_OUT} (bias); microseconds per forward, the median of {args.passes} interleaved passes of {args.reps} forwards "
                 "after a warm-up, every call issued from Python between one pair of events per pass.\n\n")
        fo.write("chain = `QMLP.forward`: `quantize(x)`, `qlinear(.., out_scale)` (int8 -> int8), `qlinear` (int8 -> fp32), three "
                 "launches; 2 qlinear = `q8.qlinear` twice, four launches (the baseline: what the library offered before); spread = "
                 "max - min of the baseline's passes; 2 linear = `MMult.linear` twice in fp32.  The chain is ahead only where it wins "
                 "by more than the spread.  max rel diff = max|chain - baseline| / max|baseline|: the hidden layer's static "
                 "quantisation against the baseline's per-row one.\n\n")
        fo.write("| rows | chain us | 2 qlinear us | spread us | chain - 2 qlinear us | ahead by more than the spread | 2 linear us | max rel diff |\n"
                 "|---|---|---|---|---|---|---|---|\n")
        for rows, ms, _, _, rel in table:
            med = {k: statistics.median(v) * 1e3 for k, v in ms.items()}
            spread = (max(ms["2 qlinear"]) - min(ms["2 qlinear"])) * 1e3
            diff = med["chain"] - med["2 qlinear"]
            fo.write(f"| {rows} | {med['chain']:.1f} | {med['2 qlinear']:.1f} | {spread:.1f} | {diff:+.1f} | "
                     f"{'yes' if -diff > spread else 'NO'} | {med['2 linear']:.1f} | {rel:.3g} |\n")
        fo.write("\nThe GEMMs alone, from rows that are quantised already (no quantiser pass in either column):\n\n")
        fo.write("| rows x out x in | s8 -> s8 us | s8 -> f32 us | s8 -> s8 - s8 -> f32 us |\n|---|---|---|---|\n")
        for rows, ms, _, _, _ in table:
            med = {k: statistics.median(v) * 1e3 for k, v in ms.items()}
            for name, n_out, n_in in (("L1", D_HID, D_IN), ("L2", D_OUT, D_HID)):
                a, b = med[f"{name} s8->s8"], med[f"{name} s8->f32"]
                fo.write(f"| {rows} x {n_out} x {n_in} | {a:.1f} | {b:.1f} | {a - b:+.1f} |\n")
        fo.write("\nLaunches:\n\n")
        for rows, _, launch1, launch2, _ in table:
            fo.write(f"- {rows} rows: layer 1 `{launch1}`; layer 2 `{launch2}`\n")
    mm.close()
    print("wrote", args.out)


if __name__ == "__main__":
    main()
