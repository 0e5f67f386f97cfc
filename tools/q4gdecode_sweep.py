#!/usr/bin/env python3
"""q4gdecode_sweep.py -- the small-batch layer on 4-bit weights with one scale per group of 128 input features
(libmmult_hip_q4g.so, q8.qlinear_decode on a QWeight4G) beside the two paths that existed before it, measured in the same run:
the same call on the QWeight4 (libmmult_hip_q4d.so, one scale per channel) and on the int8 QWeight (libmmult_hip_q8d.so) of the
same layer.  tools/q4decode_sweep.py's protocol: rows {1, 16} x (out, in) {(4096, 4096), (11008, 4096), (4096, 11008)}, both
outputs, every layer with bias and ReLU from a QRows (no quantiser pass).
  warm   mmh_time_q4g_linear beside mmh_time_q4d_linear and mmh_time_q8d_linear: `reps` calls on one weight between one pair of
         events in the library
  cold   the same call rotating through enough distinct weights to exceed the 256 MB last-level cache, one rotation captured
         in a graph and replayed (no Python between the launches): HBM-cold streaming
Every figure is microseconds per call, the median of `--passes` interleaved passes after a warm-up; the spread (max - min) of
each baseline's own passes is given, and the group path is "ahead" of the int8 path only where it wins by more than that path's
spread.  The group path streams 1/16 more bytes than the per-channel one (4 bytes of scale per 64 bytes of nibbles).
Then the accuracy table, which is what the format is for: the relative Frobenius error of the layer's output against x w^T in
float64 for the three weight formats, on a Gaussian weight and on the same weight with one element per row scaled by 20.
Writes profiles/q4gdecode_sweep.md.

    python tools/q4gdecode_sweep.py [--passes 5] [--reps 50] [--no-cold] [--out profiles/q4gdecode_sweep.md]"""
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
from q4decode_sweep import LLC_BYTES, ROWS, SHAPES, outputs  # noqa: E402

PATHS = (("w4g", q8.QWeight4G), ("w4", q8.QWeight4), ("w8", q8.QWeight))


def weight_bytes(path, out, in_):
    return {"w4g": out * in_ // 2 + -(-in_ // 128) * out * 4, "w4": out * in_ // 2, "w8": out * in_}[path]


def cold_calls(rows, out, in_, reps):
    """{(path, output): () -> ms per call} of one graph replay over enough distinct weights of each kind to exceed the
    last-level cache with that kind's own bytes."""
    x = q8.quantize(torch.randn((rows, in_), device="cuda"))
    calls, keep = {}, []
    for path, make in PATHS:
        count = LLC_BYTES // weight_bytes(path, out, in_) + 2
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


def rel(got, want):
    return float((got.double() - want).norm() / want.norm())


def accuracy(rows=16, out=4096, in_=4096):
    """[(weight, {format: (layer error, weight error)})]: the layer's fp32 output (x quantised per row, as every path does)
    against x w^T in float64, and the dequantised weight against w."""
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn((rows, in_), device="cuda", generator=g)
    plain = torch.randn((out, in_), device="cuda", generator=g) / in_ ** 0.5
    spiked = plain.clone()
    cols = torch.randint(0, in_, (out,), device="cuda", generator=g)
    spiked[torch.arange(out, device="cuda"), cols] *= 20.0
    table = []
    for name, w in (("Gaussian", plain), ("one element per row x 20", spiked)):
        want = x.double() @ w.double().t()
        row = {}
        for path, make in PATHS:
            qw = make(w)
            y = q8.qlinear_decode(x, qw)
            if path == "w4g":
                deq = qw.dequantize()
            elif path == "w4":
                deq = (qw.unpack()[:, :out].float() * qw.inv_scale).t()
            else:
                deq = (qw.q[:, :out].float() * qw.inv_scale).t()
            row[path] = (rel(y, want), rel(deq, w.double()))
            qw.close()
        table.append((name, row))
    return table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "q4gdecode_sweep.md"))
    ap.add_argument("--no-cold", action="store_true")
    args = ap.parse_args()
    mm = H.MMult(0, "auto")
    hbm = mm.probe_hbm_copy()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    warm, cold, launches = [], [], []
    for out, in_ in SHAPES:
        w = torch.randn((out, in_), device="cuda") / in_ ** 0.5
        weights = {path: make(w) for path, make in PATHS}
        del w
        for qw in weights.values():
            qw.reserve_decode()
        bias = torch.randn(out, device="cuda") * 0.1
        for rows in ROWS:
            x = q8.quantize(torch.randn((rows, in_), device="cuda"))
            calls = {}
            for name, (y, scale) in outputs(rows, out).items():
                for path, qw in weights.items():
                    calls[path, name] = (lambda qw=qw, y=y, scale=scale:
                                         q8.time_qlinear_decode(x, qw, bias, "relu", out=y, out_scale=scale, warmup=2, reps=args.reps))
            ms = passes_of(calls, args.passes)
            warm.append((rows, out, in_, ms))
            launches.append((rows, out, in_, q8.last_launch_q4g(), q8.last_launch_q4d(), q8.last_launch_q8d()))
            print(rows, out, in_, " ".join(f"{p}.{n} {med(v):.1f}us" for (p, n), v in ms.items()), flush=True)
        for qw in weights.values():
            qw.close()
        del weights
        if not args.no_cold:
            for rows in ROWS:
                calls, keep = cold_calls(rows, out, in_, 4)
                ms = passes_of(calls, args.passes)
                cold.append((rows, out, in_, ms))
                print("cold", rows, out, in_, " ".join(f"{p}.{n} {med(v):.1f}us" for (p, n), v in ms.items()), flush=True)
                del calls, keep
                torch.cuda.empty_cache()
    errors = accuracy()

    dev = "MI355X" if "gfx950" in torch.cuda.get_device_properties(0).gcnArchName else torch.cuda.get_device_properties(0).name

    def rows_of(fo, table):
        fo.write("| rows x out x in | out | group us | 4-bit us | spread | int8 us | spread | group / 4-bit | group / int8 | ahead of int8 | group GB/s | of copy |\n"
                 "|---|---|---|---|---|---|---|---|---|---|---|---|\n")
        for rows, out, in_, ms in table:
            for name in ("s8", "f32"):
                a, b, c = med(ms["w4g", name]), med(ms["w4", name]), med(ms["w8", name])
                sb, sc = spread(ms["w4", name]), spread(ms["w8", name])
                gbs = weight_bytes("w4g", out, in_) / (a * 1e-6) / 1e9
                fo.write(f"| {rows} x {out} x {in_} | {name} | {a:.1f} | {b:.1f} | {sb:.1f} | {c:.1f} | {sc:.1f} | {a / b:.2f} | {a / c:.2f} | "
                         f"{'yes' if c - a > sc else 'NO'} | {gbs:.0f} | {gbs / hbm:.2f} |\n")

    with open(args.out, "w") as fo:
        fo.write("# The small-batch layer on 4-bit weights with per-group scales (groups of 128) beside the two layers before it\n\n")
        fo.write(f"`python tools/q4gdecode_sweep.py --passes {args.passes} --reps {args.reps}` on one {dev} ({cus} CUs); microseconds per call, "
                 f"the median of {args.passes} interleaved passes after a warm-up; every layer with bias and ReLU, from a QRows.  "
                 f"mmh_probe_hbm_copy in the same session: {hbm:.0f} GB/s (read + write bytes).\n\n")
        fo.write("group: `q8.qlinear_decode` on a `QWeight4G` (libmmult_hip_q4g.so).  4-bit: the same call on the `QWeight4` of the same layer "
                 "(libmmult_hip_q4d.so), int8: on its `QWeight` (libmmult_hip_q8d.so) -- both unchanged code, in the same run.  spread = max - "
                 "min of that baseline's own passes; group / x = the group path's time over the baseline's (below 1: faster); ahead of int8 = "
                 "the group path wins by more than the int8 path's spread.  GB/s = the group path's image and scale bytes over its time.\n\n")
        fo.write("Bytes streamed per call:\n\n| out x in | int8 | 4-bit | group | group / 4-bit |\n|---|---|---|---|---|\n")
        for out, in_ in SHAPES:
            b = [weight_bytes(p, out, in_) for p in ("w8", "w4", "w4g")]
            fo.write(f"| {out} x {in_} | {b[0]} | {b[1]} | {b[2]} | {b[2] / b[1]:.4f} |\n")
        fo.write(f"\nWarm weights: the libraries' `mmh_time_*_linear` loops, {args.reps} calls on one weight between one pair of events "
                 "(the weight stays in the last-level cache):\n\n")
        rows_of(fo, warm)
        if cold:
            fo.write(f"\nCold weights: one graph replay over enough distinct weights of each kind to exceed the {LLC_BYTES >> 20} MB last-level "
                     "cache with that kind's own bytes, per call:\n\n")
            rows_of(fo, cold)
        fo.write("\nAccuracy (16 x 4096 x 4096, no timing): relative Frobenius error of the layer's fp32 output against x w^T in float64 -- x "
                 "quantised per row as every path does --, and of the dequantised weight against w:\n\n"
                 "| weight | int8 output | 4-bit output | group output | int8 weight | 4-bit weight | group weight |\n|---|---|---|---|---|---|---|\n")
        for name, row in errors:
            fo.write(f"| {name} | {row['w8'][0]:.4f} | {row['w4'][0]:.4f} | {row['w4g'][0]:.4f} | {row['w8'][1]:.4f} | {row['w4'][1]:.4f} | "
                     f"{row['w4g'][1]:.4f} |\n")
        fo.write("\nLaunches:\n\n")
        for rows, out, in_, lg, l4, l8 in launches:
            fo.write(f"- {rows} x {out} x {in_}: `{lg}` beside `{l4}` and `{l8}`\n")
    mm.close()
    print("wrote", args.out)


if __name__ == "__main__":
    main()
