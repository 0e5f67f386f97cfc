#!/usr/bin/env python3
"""q4decode_sweep.py -- the small-batch layer on 4-bit weights (libmmult_hip_q4d.so, q8.qlinear_decode on a QWeight4) beside the
same call on the int8 QWeight of the same layer (libmmult_hip_q8d.so, unchanged code, measured in the same run), at decode
shapes: rows {1, 16} x (out, in) {(4096, 4096), (11008, 4096), (4096, 11008)}, both outputs, every layer with bias and ReLU from
a QRows (no quantiser pass).
  warm   mmh_time_q4d_linear beside mmh_time_q8d_linear: `reps` calls on one weight between one pair of events in the library
  cold   the same call rotating through enough distinct weights to exceed the 256 MB last-level cache, one rotation captured
         in a graph and replayed (no Python between the launches): HBM-cold streaming
Every figure is microseconds per call, the median of `--passes` interleaved passes after a warm-up (tools/qdecode_sweep.py's
protocol); the spread (max - min) of the int8 baseline's own passes is the yardstick: 4 bits is "ahead" only where it wins by
more than that.  Also recorded: the two images' bytes, and each path's GB/s of its own image.  Writes profiles/q4decode_sweep.md.

    python tools/q4decode_sweep.py [--passes 5] [--reps 50] [--out profiles/q4decode_sweep.md]"""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
import how_to_optimize_gemm_amd as H  # noqa: E402
from how_to_optimize_gemm_amd import q8  # noqa: E402
from qdecode_sweep import events, med, passes_of, spread  # noqa: E402

ROWS = (1, 16)
SHAPES = ((4096, 4096), (11008, 4096), (4096, 11008))
LLC_BYTES = 256 << 20


def outputs(rows, out):
    """{name: (out tensor, out_scale)} of the two output forms."""
    return {"s8": (torch.empty((rows, (out + 15) & ~15), dtype=torch.int8, device="cuda")[:, :out], 1.0),
            "f32": (torch.empty((rows, out), device="cuda"), None)}


def cold_calls(rows, out, in_, reps):
    """{(path, output): () -> ms per call} of one graph replay over enough distinct weights of each kind to exceed the
    last-level cache with that kind's own images."""
    x = q8.quantize(torch.randn((rows, in_), device="cuda"))
    calls, keep = {}, []
    for path, make, nbytes in (("w4", q8.QWeight4, out * in_ // 2), ("w8", q8.QWeight, out * in_)):
        count = LLC_BYTES // nbytes + 2
        weights = []
        for _ in range(count):
            w = torch.randn((out, in_), device="cuda")
            weights.append(make(w))
            del w
        for qw in weights:
            qw.reserve_decode()
        keep.append(weights)
        for name, (y, scale) in outputs(rows, out).items():
            so = inv = None
            if scale is not None:
                so, inv = q8._scale_vectors("sweep", scale, rows, 0)
            for qw in weights:
                q8._linear_q8d("sweep", x, qw, None, None, so, inv, y)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                for qw in weights:
                    q8._linear_q8d("sweep", x, qw, None, None, so, inv, y)
            keep.append((g, y, so, inv))
            calls[path, name] = (lambda g=g, count=count: events(g.replay, reps, 1) / count)
    return calls, keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "q4decode_sweep.md"))
    ap.add_argument("--no-cold", action="store_true")
    args = ap.parse_args()
    mm = H.MMult(0, "auto")
    hbm = mm.probe_hbm_copy()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    warm, cold, sizes, launches = [], [], [], []
    for out, in_ in SHAPES:
        w = torch.randn((out, in_), device="cuda") / in_ ** 0.5
        qw8, qw4 = q8.QWeight(w), q8.QWeight4(w)
        del w
        qw8.reserve_decode()
        qw4.reserve_decode()
        sizes.append((out, in_, in_ * qw8.pitch, qw4.nbytes))
        bias = torch.randn(out, device="cuda") * 0.1
        for rows in ROWS:
            x = q8.quantize(torch.randn((rows, in_), device="cuda"))
            calls = {}
            for name, (y, scale) in outputs(rows, out).items():
                for path, qw in (("w4", qw4), ("w8", qw8)):
                    calls[path, name] = (lambda qw=qw, y=y, scale=scale:
                                         q8.time_qlinear_decode(x, qw, bias, "relu", out=y, out_scale=scale, warmup=2, reps=args.reps))
            ms = passes_of(calls, args.passes)
            warm.append((rows, out, in_, ms))
            launches.append((rows, out, in_, q8.last_launch_q4d(), q8.last_launch_q8d()))
            print(rows, out, in_, " ".join(f"{p}.{n} {med(v):.1f}us" for (p, n), v in ms.items()), flush=True)
        qw8.close()
        del qw8, qw4
        if not args.no_cold:
            for rows in ROWS:
                calls, keep = cold_calls(rows, out, in_, 4)
                ms = passes_of(calls, args.passes)
                cold.append((rows, out, in_, ms))
                print("cold", rows, out, in_, " ".join(f"{p}.{n} {med(v):.1f}us" for (p, n), v in ms.items()), flush=True)
                del calls, keep
                torch.cuda.empty_cache()

    dev = "MI355X" if "gfx950" in torch.cuda.get_device_properties(0).gcnArchName else torch.cuda.get_device_properties(0).name

    def rows_of(fo, table):
        fo.write("| rows x out x in | out | 4-bit us | int8 us | spread us | ahead | int8 / 4-bit | 4-bit GB/s | of copy | int8 GB/s | of copy |\n"
                 "|---|---|---|---|---|---|---|---|---|---|---|\n")
        for rows, out, in_, ms in table:
            for name in ("s8", "f32"):
                a, b, sp = med(ms["w4", name]), med(ms["w8", name]), spread(ms["w8", name])
                g4, g8 = out * in_ / 2 / (a * 1e-6) / 1e9, out * in_ / (b * 1e-6) / 1e9
                fo.write(f"| {rows} x {out} x {in_} | {name} | {a:.1f} | {b:.1f} | {sp:.1f} | {'yes' if b - a > sp else 'NO'} | {b / a:.2f} | "
                         f"{g4:.0f} | {g4 / hbm:.2f} | {g8:.0f} | {g8 / hbm:.2f} |\n")

    with open(args.out, "w") as fo:
        fo.write("# The small-batch layer on 4-bit weights (W4A8) beside the int8 layer\n\n")
        fo.write(f"`python tools/q4decode_sweep.py --passes {args.passes} --reps {args.reps}` on one {dev} ({cus} CUs); microseconds per call, the "
                 f"median of {args.passes} interleaved passes after a warm-up; every layer with bias and ReLU, from a QRows.  "
                 f"mmh_probe_hbm_copy in the same session: {hbm:.0f} GB/s (read + write bytes).\n\n")
        fo.write("4-bit: `q8.qlinear_decode` on a `QWeight4` (libmmult_hip_q4d.so).  int8: the same call on the `QWeight` of the same layer "
                 "(libmmult_hip_q8d.so, unchanged code), in the same run.  spread = max - min of the int8 path's passes; ahead = 4 bits wins by "
                 "more than that.  GB/s = each path's OWN image bytes over its time; of copy = that over mmh_probe_hbm_copy's rate.\n\n")
        fo.write("The images:\n\n| out x in | int8 image bytes | 4-bit image bytes | ratio |\n|---|---|---|---|\n")
        for out, in_, b8, b4 in sizes:
            fo.write(f"| {out} x {in_} | {b8} | {b4} | {b4 / b8:.3f} |\n")
        fo.write(f"\nWarm weights: `mmh_time_q4d_linear` beside `mmh_time_q8d_linear`, {args.reps} calls on one weight between one pair of "
                 "events in the library (the weight stays in the last-level cache):\n\n")
        rows_of(fo, warm)
        if cold:
            fo.write(f"\nCold weights: one graph replay over enough distinct weights of each kind to exceed the {LLC_BYTES >> 20} MB last-level "
                     "cache with that kind's own images, per call:\n\n")
            rows_of(fo, cold)
        fo.write("\nLaunches:\n\n")
        for rows, out, in_, l4, l8 in launches:
            fo.write(f"- {rows} x {out} x {in_}: `{l4}` beside `{l8}`\n")
    mm.close()
    print("wrote", args.out)


if __name__ == "__main__":
    main()
