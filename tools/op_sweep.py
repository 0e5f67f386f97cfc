#!/usr/bin/env python3
"""op_sweep.py -- the transposed-operand forms against NN on MMH_KERNEL_AUTO: C = op(A) op(B) for NT / TN / TT beside
C = A B on the same shape, each timed by mmh_time_sgemm_op (calls issued from C, one event pair per burst), in
interleaved bursts after a warm-up, on the 25 reference sizes (1024 .. 4096 step 128) and ten off-grid shapes from
tools/policy_shapes_heldout.txt.  Writes profiles/op_sweep.md: TFLOP/s per form (median burst), op / NN and the family
each launched.

    python tools/op_sweep.py [--bursts 7] [--reps 10] [--out profiles/op_sweep.md]"""
import argparse
import os
import re
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402
import how_to_optimize_gemm_amd as H  # noqa: E402

FORMS = [("NN", 0, 0), ("NT", 0, 1), ("TN", 1, 0), ("TT", 1, 1)]


def heldout(count):
    rows = []
    for line in open(os.path.join(REPO, "tools", "policy_shapes_heldout.txt")):
        line = line.strip()
        if line and not line.startswith("#"):
            rows.append(tuple(int(x) for x in line.split(",")[:3]))
    step = max(1, len(rows) // count)
    return rows[::step][:count]


def family(launch):
    m = re.match(r"(\w+)<(\d+),(\d+)>", launch)
    if not m:
        return launch.split(" ")[0]
    form = "sk" if "persistent" in launch else "plain"
    return f"{m.group(2)}x{m.group(3)} {form}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bursts", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "op_sweep.md"))
    args = ap.parse_args()
    mm = H.MMult(0, "auto")
    stream = torch.cuda.current_stream().cuda_stream
    shapes = [(n, n, n) for n in range(1024, 4097, 128)] + heldout(10)
    rows = []
    for (m, n, k) in shapes:
        a = torch.rand((m, k), device="cuda") - 0.5
        b = torch.rand((k, n), device="cuda") - 0.5
        at, bt = a.t().contiguous(), b.t().contiguous()
        c = torch.empty((m, n), device="cuda")
        stored = {0: (a, k), 1: (at, m)}, {0: (b, n), 1: (bt, k)}
        ms = {f: [] for f, _, _ in FORMS}
        launched = {}

        def run(f, ta, tb, reps, warm):
            (pa, lda), (pb, ldb) = stored[0][ta], stored[1][tb]
            t = mm.time_sgemm_op(ta, tb, m, n, k, pa.data_ptr(), lda, pb.data_ptr(), ldb, c.data_ptr(), n, warm, reps, stream)
            launched[f] = H.last_launch()
            return t

        for f, ta, tb in FORMS:
            run(f, ta, tb, 3, 3)
        for _ in range(args.bursts):
            for f, ta, tb in FORMS:
                ms[f].append(run(f, ta, tb, args.reps, 0))
        tf = {f: 2.0 * m * n * k / (statistics.median(v) * 1e-3) / 1e12 for f, v in ms.items()}
        rows.append((m, n, k, tf, {f: family(launched[f]) for f in launched}))
        print(m, n, k, " ".join(f"{f} {tf[f]:.1f}" for f, _, _ in FORMS), launched["NN"].split(",")[0], flush=True)
        del a, b, at, bt, c
    dev = "MI355X" if "gfx950" in torch.cuda.get_device_properties(0).gcnArchName else torch.cuda.get_device_properties(0).name
    with open(args.out, "w") as fo:
        fo.write("# Transposed operands against NN (MMH_KERNEL_AUTO)\n\n")
        fo.write(f"`python tools/op_sweep.py --bursts {args.bursts} --reps {args.reps}` on one {dev}: every form timed by "
                 "mmh_time_sgemm_op in interleaved bursts after a warm-up, TFLOP/s of the median burst.  Family: the tile and "
                 "launch form each call ran (NN's may be outside the three tiles with op forms).\n\n")
        fo.write("| m | n | k | NN TF/s | NT | TN | TT | NT/NN | TN/NN | TT/NN | NN family | op family |\n")
        fo.write("|---|---|---|---|---|---|---|---|---|---|---|---|\n")
        for (m, n, k, tf, fam) in rows:
            opf = sorted(set(fam[f] for f in ("NT", "TN", "TT")))
            fo.write(f"| {m} | {n} | {k} | {tf['NN']:.1f} | {tf['NT']:.1f} | {tf['TN']:.1f} | {tf['TT']:.1f} | "
                     f"{tf['NT'] / tf['NN']:.3f} | {tf['TN'] / tf['NN']:.3f} | {tf['TT'] / tf['NN']:.3f} | {fam['NN']} | "
                     f"{' / '.join(opf)} |\n")
    mm.close()
    print("wrote", args.out)


if __name__ == "__main__":
    main()
