#!/usr/bin/env python3
"""qdecode_sweep.py -- the small-batch int8 layer (libmmult_hip_q8d.so, q8.qlinear_decode) beside the tile path, at decode
shapes: rows {1, 8, 16} x (out, in) {(4096, 4096), (11008, 4096), (4096, 11008)}, every layer from a QRows (no quantiser pass).
  int8 out   mmh_time_q8d_linear beside mmh_time_q8o_linear (both time `reps` calls between one pair of events in the library)
  fp32 out   q8.qlinear_decode beside q8.qlinear(QRows), both issued from Python between one pair of events per pass
  GB/s       the weight's bytes over the int8-output time, beside mmh_probe_hbm_copy's rate of the same session
  cold       the same call rotating through enough distinct QWeights to exceed the 256 MB last-level cache, one rotation
             captured in a graph and replayed (so that no Python sits between the launches): HBM-cold streaming
  chain      QMLP 4096 -> 11008 -> 4096 at 16 rows with decode=True beside decode=False, issued from Python
  fit        forced split counts at 16 rows: what qdecode_plan.hpp's occupancy target and traffic bound were fitted on
Every figure is the median of `--passes` interleaved passes after a warm-up (tools/qlinear_sweep.py's protocol); the spread
(max - min) of the baseline's own passes is the yardstick: the new path is "ahead" only where it wins by more than that.
Writes profiles/qdecode_sweep.md.

    python tools/qdecode_sweep.py [--passes 5] [--reps 50] [--out profiles/qdecode_sweep.md]"""
import argparse
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402
import how_to_optimize_gemm_amd as H  # noqa: E402
from how_to_optimize_gemm_amd import q8  # noqa: E402

ROWS = (1, 8, 16)
SHAPES = ((4096, 4096), (11008, 4096), (4096, 11008))
LLC_BYTES = 256 << 20
FIT_SPLITS = (1, 2, 4, 8, 12, 16, 24, 32, 43)


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


def passes_of(calls, passes):
    """{name: [ms per pass]} of `passes` interleaved passes over calls = {name: () -> ms}; one warm-up round first."""
    for f in calls.values():
        f()
    ms = {name: [] for name in calls}
    for _ in range(passes):
        for name, f in calls.items():
            ms[name].append(f())
    return ms


def med(v):
    return statistics.median(v) * 1e3


def spread(v):
    return (max(v) - min(v)) * 1e3


def cold_calls(rows, out, in_, reps):
    """() -> ms per call of one graph replay over enough distinct weights to exceed the last-level cache, for both paths."""
    count = LLC_BYTES // (out * in_) + 2
    x = q8.quantize(torch.randn((rows, in_), device="cuda"))
    so, inv = q8._scale_vectors("sweep", 1.0, rows, 0)
    yq = torch.empty((rows, (out + 15) & ~15), dtype=torch.int8, device="cuda")[:, :out]
    weights = []
    for _ in range(count):
        w = torch.randn((out, in_), device="cuda")
        weights.append(q8.QWeight(w))
        del w
    for qw in weights:
        qw.reserve_decode()
    graphs = {}
    for name, layer in (("decode", q8._linear_q8d), ("tile", q8._linear_s8o)):
        for qw in weights:
            layer("sweep", x, qw, None, None, so, inv, yq)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for qw in weights:
                layer("sweep", x, qw, None, None, so, inv, yq)
        graphs[name] = g
    calls = {name: (lambda g=g: events(g.replay, reps, 1) / count) for name, g in graphs.items()}
    return calls, weights, count


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "qdecode_sweep.md"))
    ap.add_argument("--no-cold", action="store_true")
    args = ap.parse_args()
    mm = H.MMult(0, "auto")
    hbm = mm.probe_hbm_copy()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    table, fit, cold = [], [], []
    for out, in_ in SHAPES:
        qw = q8.QWeight(torch.randn((out, in_), device="cuda") / in_ ** 0.5)
        qw.reserve_decode()
        bias = torch.randn(out, device="cuda") * 0.1
        for rows in ROWS:
            x = q8.quantize(torch.randn((rows, in_), device="cuda"))
            yf = torch.empty((rows, out), device="cuda")
            calls = {
                "d8": lambda: q8.time_qlinear_decode(x, qw, bias, "relu", out_scale=1.0, warmup=2, reps=args.reps),
                "t8": lambda: q8.time_qlinear_s8o(x, qw, bias, "relu", out_scale=1.0, warmup=2, reps=args.reps),
                "df": lambda: events(lambda: q8.qlinear_decode(x, qw, bias, "relu", out=yf), args.reps, 3),
                "tf": lambda: events(lambda: q8.qlinear(x, qw, bias, "relu", out=yf), args.reps, 3),
            }
            ms = passes_of(calls, args.passes)
            q8.qlinear_decode(x, qw, bias, "relu", out_scale=1.0)
            table.append((rows, out, in_, ms, q8.last_launch_q8d()))
            print(rows, out, in_, " ".join(f"{k} {med(v):.1f}us" for k, v in ms.items()), flush=True)
            if rows == 16:
                row = {}
                slices = (in_ + 127) // 128
                for s in FIT_SPLITS:
                    if (s - 1) * 128 * ((slices + s - 1) // s) < in_:   # (no K range is empty)
                        qw._decode_workspace(q8.qlinear_decode_plan(rows, out, in_, pitch_n=qw.pitch, splits=s, cu_count=cus)[1])
                        row[s] = statistics.median(q8.time_qlinear_decode(x, qw, bias, "relu", out_scale=1.0, splits=s, warmup=2, reps=args.reps)
                                                   for _ in range(args.passes)) * 1e3
                fit.append((out, in_, row))
                print("fit", out, in_, row, flush=True)
        qw.close()
        del qw
        if not args.no_cold:
            calls, weights, count = cold_calls(16, out, in_, 4)
            ms = passes_of(calls, args.passes)
            cold.append((16, out, in_, count, ms))
            print("cold", out, in_, count, " ".join(f"{k} {med(v):.1f}us" for k, v in ms.items()), flush=True)
            for w in weights:
                w.close()
            del calls, weights
            torch.cuda.empty_cache()
    # the two-layer chain at 16 rows
    d_in, d_hid = 4096, 11008
    w1, w2 = torch.randn((d_hid, d_in), device="cuda") / d_in ** 0.5, torch.randn((d_in, d_hid), device="cuda") / d_hid ** 0.5
    b1, b2 = torch.randn(d_hid, device="cuda") * 0.1, torch.randn(d_in, device="cuda") * 0.1
    qws = [q8.QWeight(w1), q8.QWeight(w2)]
    x = torch.randn((16, d_in), device="cuda")
    tile, dec = q8.QMLP(qws, [b1, b2]), q8.QMLP(qws, [b1, b2], decode=True)
    dec.out_scales = tile.calibrate(x)
    for qw in qws:
        qw.reserve_decode()
    same = bool(torch.equal(tile(x).view(torch.int32), dec(x).view(torch.int32)))
    chain = passes_of({"decode": lambda: events(lambda: dec(x), args.reps, 3), "tile": lambda: events(lambda: tile(x), args.reps, 3)}, args.passes)
    print("chain", " ".join(f"{k} {med(v):.1f}us" for k, v in chain.items()), "same bits" if same else "DIFFERENT BITS", flush=True)

    dev = "MI355X" if "gfx950" in torch.cuda.get_device_properties(0).gcnArchName else torch.cuda.get_device_properties(0).name
    with open(args.out, "w") as fo:
        fo.write("# The small-batch int8 layer (split-K decode kernels) beside the tile path\n\n")
        fo.write(f"`python tools/qdecode_sweep.py --passes {args.passes} --reps {args.reps}` on one {dev} ({cus} CUs); microseconds per call, the "
                 f"median of {args.passes} interleaved passes of {args.reps} calls after a warm-up; every layer with bias and ReLU, from a "
                 f"QRows.  mmh_probe_hbm_copy in the same session: {hbm:.0f} GB/s (read + write bytes).\n\n")
        fo.write("int8 out: `mmh_time_q8d_linear` (decode) beside `mmh_time_q8o_linear` (tile), timed in the library.  fp32 out: "
                 "`q8.qlinear_decode` beside `q8.qlinear(QRows)`, both issued from Python.  spread = max - min of the tile path's passes; "
                 "ahead = the decode path wins by more than that.  GB/s = out x in bytes of weight over the decode int8 time; of copy = that "
                 "over mmh_probe_hbm_copy's rate.\n\n")
        fo.write("| rows x out x in | decode s8 us | tile s8 us | spread us | ahead | GB/s | of copy | decode f32 us | tile f32 us | spread us | ahead |\n"
                 "|---|---|---|---|---|---|---|---|---|---|---|\n")
        for rows, out, in_, ms, _ in table:
            gbs = out * in_ / (med(ms["d8"]) * 1e-6) / 1e9
            fo.write(f"| {rows} x {out} x {in_} | {med(ms['d8']):.1f} | {med(ms['t8']):.1f} | {spread(ms['t8']):.1f} | "
                     f"{'yes' if med(ms['t8']) - med(ms['d8']) > spread(ms['t8']) else 'NO'} | {gbs:.0f} | {gbs / hbm:.2f} | "
                     f"{med(ms['df']):.1f} | {med(ms['tf']):.1f} | {spread(ms['tf']):.1f} | "
                     f"{'yes' if med(ms['tf']) - med(ms['df']) > spread(ms['tf']) else 'NO'} |\n")
        if cold:
            fo.write(f"\nCold weights: int8 out at 16 rows, one graph replay over `count` distinct QWeights (more than the {LLC_BYTES >> 20} MB "
                     "last-level cache), per call:\n\n")
            fo.write("| rows x out x in | count | decode us | tile us | spread us | ahead | GB/s | of copy |\n|---|---|---|---|---|---|---|---|\n")
            for rows, out, in_, count, ms in cold:
                gbs = out * in_ / (med(ms["decode"]) * 1e-6) / 1e9
                fo.write(f"| {rows} x {out} x {in_} | {count} | {med(ms['decode']):.1f} | {med(ms['tile']):.1f} | {spread(ms['tile']):.1f} | "
                         f"{'yes' if med(ms['tile']) - med(ms['decode']) > spread(ms['tile']) else 'NO'} | {gbs:.0f} | {gbs / hbm:.2f} |\n")
        fo.write(f"\nThe two-layer chain 16 x {d_in} -> {d_hid} -> {d_in} (`QMLP.forward`, issued from Python; profiles/qchain_sweep.md has the tile "
                 f"path's at 79.1 us): decode=True {med(chain['decode']):.1f} us, decode=False {med(chain['tile']):.1f} us (spread "
                 f"{spread(chain['tile']):.1f} us), {'the same bits' if same else 'DIFFERENT BITS'}.\n")
        fo.write("\nThe fit: forced split counts at 16 rows (int8 out, us), behind qdecode_plan.hpp's occupancy target and traffic bound:\n\n")
        fo.write("| out x in | " + " | ".join(f"{s} splits" for s in FIT_SPLITS) + " |\n|---|" + "---|" * len(FIT_SPLITS) + "\n")
        for out, in_, row in fit:
            fo.write(f"| {out} x {in_} | " + " | ".join(f"{row[s]:.1f}" if s in row else "-" for s in FIT_SPLITS) + " |\n")
        fo.write("\nLaunches:\n\n")
        for rows, out, in_, _, launch in table:
            fo.write(f"- {rows} x {out} x {in_}: `{launch}`\n")
    mm.close()
    print("wrote", args.out)


if __name__ == "__main__":
    main()
