#!/usr/bin/env python3
"""qlinear_sweep.py -- the int8 linear layer (q8.qlinear: weight prepared once, activations quantised per row, fused epilogue)
beside what it replaces and beside fp32, at four layer shapes (rows x out x in).
  qlinear   q8.qlinear(x, qweight)                       the row quantiser + the int8 GEMM with its epilogue
  qgemm     MMult.qgemm(x, wt), wt the materialised in x out weight: quantises BOTH operands per tensor on every call
  linear    MMult.linear(x, w) in fp32
  quantiser q8.quantize_rows(x) alone, in GB/s counted as rows in (4 + 1) bytes, beside mmh_probe_hbm_copy's rate
Every call is issued from Python between one pair of events per pass; every figure is the median of `--passes` interleaved
passes after a warm-up, and qgemm's spread (max - min of its passes) is the yardstick of the acceptance column: qlinear is
not slower than qgemm by more than that spread.  Writes profiles/qlinear_sweep.md.

    python tools/qlinear_sweep.py [--passes 5] [--reps 20] [--out profiles/qlinear_sweep.md]"""
import argparse
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402
import how_to_optimize_gemm_amd as H  # noqa: E402
from how_to_optimize_gemm_amd import q8  # noqa: E402

SHAPES = [(16, 4096, 4096), (512, 4096, 4096), (4096, 4096, 4096), (4096, 11008, 4096)]   # rows x out x in


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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "qlinear_sweep.md"))
    args = ap.parse_args()
    mm = H.MMult(0, "auto")
    hbm = mm.probe_hbm_copy()
    table = []
    for rows, n_out, n_in in SHAPES:
        x = torch.randn((rows, n_in), device="cuda")
        w = torch.randn((n_out, n_in), device="cuda") / n_in ** 0.5
        wt = w.t().contiguous()
        qw = q8.QWeight(w)
        y, yq, yf = (torch.empty((rows, n_out), device="cuda") for _ in range(3))
        xq = torch.empty((rows, n_in), dtype=torch.int8, device="cuda")
        calls = {
            "qlinear": lambda: q8.qlinear(x, qw, out=y),
            "qgemm": lambda: mm.qgemm(x, wt, out=yq),
            "linear": lambda: mm.linear(x, w, out=yf),
            "quantiser": lambda: q8.quantize_rows(x, out=xq),
        }
        ms = passes_of(calls, args.passes, args.reps)
        q8.qlinear(x, qw, out=y)
        launch = q8.last_launch()
        mm.qgemm(x, wt, out=yq)
        table.append((rows, n_out, n_in, ms, launch, H.last_launch()))
        print(rows, n_out, n_in, " ".join(f"{k} {statistics.median(v) * 1e3:.1f}us" for k, v in ms.items()), flush=True)
        del x, w, wt, qw, y, yq, yf, xq
    dev = "MI355X" if "gfx950" in torch.cuda.get_device_properties(0).gcnArchName else torch.cuda.get_device_properties(0).name
    with open(args.out, "w") as fo:
        fo.write("# The int8 linear layer beside the per-tensor quantised GEMM and the fp32 layer\n\n")
        fo.write(f"`python tools/qlinear_sweep.py --passes {args.passes} --reps {args.reps}` on one {dev}: microseconds per call, the "
                 f"median of {args.passes} interleaved passes of {args.reps} calls after a warm-up, every call issued from Python "
                 f"between one pair of events per pass.  mmh_probe_hbm_copy in the same session: {hbm:.0f} GB/s (read + write bytes).\n\n")
        fo.write("qlinear = `q8.qlinear(x, qweight)`; qgemm = `MMult.qgemm(x, wt)` with `wt` the materialised in x out weight (what "
                 "qlinear replaces: both operands quantised per tensor on every call); spread = max - min of qgemm's passes; linear = "
                 "`MMult.linear(x, w)` in fp32; quantiser = `q8.quantize_rows(x)` alone, GB/s counted as rows x in x 5 bytes.  "
                 "Acceptance: qlinear - qgemm <= spread.\n\n")
        fo.write("| rows | out | in | qlinear us | qgemm us | qgemm spread us | qlinear - qgemm us | accepted | TOP/s (2 rows out in) | "
                 "linear us | quantiser us | quantiser GB/s | of the copy rate |\n|---|---|---|---|---|---|---|---|---|---|---|---|---|\n")
        for rows, n_out, n_in, ms, _, _ in table:
            med = {k: statistics.median(v) * 1e3 for k, v in ms.items()}
            spread = (max(ms["qgemm"]) - min(ms["qgemm"])) * 1e3
            gbs = rows * n_in * 5 / 1e9 / (med["quantiser"] * 1e-6)
            fo.write(f"| {rows} | {n_out} | {n_in} | {med['qlinear']:.1f} | {med['qgemm']:.1f} | {spread:.1f} | "
                     f"{med['qlinear'] - med['qgemm']:+.1f} | {'yes' if med['qlinear'] - med['qgemm'] <= spread else 'NO'} | "
                     f"{2.0 * rows * n_out * n_in / (med['qlinear'] * 1e-6) / 1e12:.0f} | {med['linear']:.1f} | {med['quantiser']:.1f} | "
                     f"{gbs:.0f} | {gbs / hbm:.2f} |\n")
        fo.write("\nLaunches:\n\n")
        for rows, n_out, n_in, _, launch, qlaunch in table:
            fo.write(f"- {rows} x {n_out} x {n_in}: qlinear `{launch}`; qgemm `{qlaunch}`\n")
    mm.close()
    print("wrote", args.out)


if __name__ == "__main__":
    main()
