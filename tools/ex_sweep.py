#!/usr/bin/env python3
"""ex_sweep.py -- the fused epilogue (mmh_sgemm_ex) against the plain call (mmh_sgemm_op) on MMH_KERNEL_AUTO, NN and NT:
(a) C = relu(op(A) op(B) + bias[j])            beta = 0: C is written only
(b) C = 0.7 op(A) op(B) + 0.5 C                reads C at the end of every tile
each timed by mmh_time_sgemm_ex / mmh_time_sgemm_op (calls issued from C, one event pair per burst) in interleaved bursts
after a warm-up, plus the unfused sequence form (a) replaces -- matmul(out=y), y.add_(bias), y.relu_() on one stream, events
around `reps` repetitions -- beside MMult.linear / MMult.addmm timed the same way.  Writes profiles/ex_sweep.md: TFLOP/s of
the median burst (2 m n k flops for every form), ratios to the plain call, and the time of the unfused sequence over the
fused call's.

    python tools/ex_sweep.py [--bursts 7] [--reps 10] [--out profiles/ex_sweep.md]"""
import argparse
import os
import re
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402
import how_to_optimize_gemm_amd as H  # noqa: E402

FORMS = [("NN", 0, 0), ("NT", 0, 1)]
SHAPES = [(n, n, n) for n in (1024, 2048, 2176, 2688, 3200, 4096)] + [(4096, 4096, 512)]


def family(launch):
    m = re.match(r"(\w+)<(\d+),(\d+)>", launch)
    if not m:
        return launch.split(" ")[0]
    return f"{m.group(2)}x{m.group(3)} {'sk' if 'persistent' in launch else 'plain'}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bursts", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ex_sweep.md"))
    args = ap.parse_args()
    mm = H.MMult(0, "auto")
    stream = torch.cuda.current_stream().cuda_stream
    rows = []
    for (m, n, k) in SHAPES:
        a = torch.rand((m, k), device="cuda") - 0.5
        b = torch.rand((k, n), device="cuda") - 0.5
        bt = b.t().contiguous()
        bias = torch.rand((n,), device="cuda") - 0.5
        c = torch.zeros((m, n), device="cuda")
        for f, ta, tb in FORMS:
            pb, ldb = (bt, k) if tb else (b, n)
            launched = {}

            def op(reps, warm):
                t = mm.time_sgemm_op(ta, tb, m, n, k, a.data_ptr(), k, pb.data_ptr(), ldb, c.data_ptr(), n, warm, reps, stream)
                launched["op"] = H.last_launch()
                return t

            def ex_a(reps, warm):
                t = mm.time_sgemm_ex(ta, tb, m, n, k, 1.0, a.data_ptr(), k, pb.data_ptr(), ldb, 0.0, c.data_ptr(), n, bias.data_ptr(),
                                     H.BIAS_COL, H.ACT_RELU, warm, reps, stream)
                launched["a"] = H.last_launch()
                return t

            def ex_b(reps, warm):
                t = mm.time_sgemm_ex(ta, tb, m, n, k, 0.7, a.data_ptr(), k, pb.data_ptr(), ldb, 0.5, c.data_ptr(), n, 0, H.BIAS_NONE,
                                     H.ACT_NONE, warm, reps, stream)
                launched["b"] = H.last_launch()
                return t

            def events(step):
                def run(reps, warm):
                    for _ in range(warm):
                        step()
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record()
                    for _ in range(reps):
                        step()
                    t1.record()
                    t1.synchronize()
                    return t0.elapsed_time(t1) / reps
                return run

            w_op = bt.t() if tb else b   # the operand as matmul / linear take it

            def unfused_step():
                mm.matmul(a, w_op, out=c)
                c.add_(bias)
                c.relu_()

            def fused_step():
                if tb:
                    mm.linear(a, bt, bias, activation="relu", out=c)
                else:
                    mm._ex("linear", a, b, c, 1.0, 0.0, bias, H.BIAS_COL, H.ACT_RELU)

            calls = {"op": op, "a": ex_a, "b": ex_b, "unfused": events(unfused_step), "fused": events(fused_step)}
            ms = {name: [] for name in calls}
            for fn in calls.values():
                fn(3, 3)
            for _ in range(args.bursts):
                for name, fn in calls.items():
                    ms[name].append(fn(args.reps, 0))
            med = {name: statistics.median(v) for name, v in ms.items()}
            tf = {name: 2.0 * m * n * k / (t * 1e-3) / 1e12 for name, t in med.items()}
            rows.append((m, n, k, f, med, tf, family(launched["op"]), family(launched["a"])))
            print(m, n, k, f, " ".join(f"{name} {med[name] * 1e3:.1f}us" for name in calls), launched["a"].split(",")[0], flush=True)
            c.zero_()   # (form (b) feeds C back into itself: keep it finite from shape to shape)
        del a, b, bt, c
    dev = "MI355X" if "gfx950" in torch.cuda.get_device_properties(0).gcnArchName else torch.cuda.get_device_properties(0).name
    with open(args.out, "w") as fo:
        fo.write("# The fused epilogue against the plain call (MMH_KERNEL_AUTO)\n\n")
        fo.write(f"`python tools/ex_sweep.py --bursts {args.bursts} --reps {args.reps}` on one {dev}: interleaved bursts after a warm-up, "
                 "the median burst of each.  plain = mmh_time_sgemm_op; (a) = mmh_time_sgemm_ex with beta = 0, a column bias and ReLU; "
                 "(b) = alpha = 0.7, beta = 0.5 (reads C); TFLOP/s count 2 m n k for every form.  unfused = matmul(out=y), y.add_(bias), "
                 "y.relu_() on one stream; fused = the same layer through MMult.linear (NT) / mmh_sgemm_ex (NN) -- both timed with events "
                 f"around {args.reps} repetitions issued from Python.\n\n")
        fo.write("| m | n | k | op | plain TF/s | (a) TF/s | (b) TF/s | (a)/plain | (b)/plain | unfused us | fused us | fused/unfused | plain family | ex family |\n")
        fo.write("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|\n")
        for (m, n, k, f, med, tf, fam_op, fam_ex) in rows:
            fo.write(f"| {m} | {n} | {k} | {f} | {tf['op']:.1f} | {tf['a']:.1f} | {tf['b']:.1f} | {tf['a'] / tf['op']:.3f} | "
                     f"{tf['b'] / tf['op']:.3f} | {med['unfused'] * 1e3:.1f} | {med['fused'] * 1e3:.1f} | "
                     f"{med['fused'] / med['unfused']:.3f} | {fam_op} | {fam_ex} |\n")
    mm.close()
    print("wrote", args.out)


if __name__ == "__main__":
    main()
