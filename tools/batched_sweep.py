#!/usr/bin/env python3
"""batched_sweep.py -- strided batched SGEMM (mmh_sgemm_batched) on one GPU: TFLOP/s of MMH_KERNEL_AUTO against a loop of
mmh_sgemm_op calls on the same matrices and against torch.bmm on the same tensors (the BLAS bundled in torch's wheel, not
this library), plus the A/B of the batched launch's raster -- XCD-contiguous runs (the product) against the plain
batch-major order -- in a child process on the tools build (libmmult_hip_ab.so, option 108).  Interleaved bursts, best
of each.  Writes profiles/batched_sweep.md.

    python tools/batched_sweep.py [--quick] [--out profiles/batched_sweep.md]
    python tools/batched_sweep.py --raster-ab        (the child: prints one JSON line per shape)
    python tools/batched_sweep.py --ex [--commit ID] [--out profiles/batched_ex_sweep.md]

--ex: the fused batched epilogue (mmh_sgemm_batched_ex on AUTO) against what it replaces -- MMult.bmm followed by torch's
in-place elementwise passes for the same result -- and against the plain mmh_sgemm_batched as the floor, for
alpha A B + beta C and for column bias + ReLU.  Event timing after warm-up, the three variants interleaved in every pass,
median and spread (max - min) over the passes.  Writes profiles/batched_ex_sweep.md."""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SHAPES = [(b, s, s, s) for b in (8, 64, 512) for s in (128, 256, 512, 1024)] + [(2, 4096, 4096, 4096), (32, 128, 4096, 128)]
RASTER_SHAPES = [(512, 128, 128, 128), (64, 512, 512, 512), (16, 1024, 1024, 1024)]
OPT_BATCH_MAJOR = 108   # tools build only


def tflops(batch, m, n, k, ms):
    return 2.0 * batch * m * n * k / (ms * 1e-3) / 1e12


def operands(batch, m, n, k):
    import torch
    g = torch.Generator(device="cuda").manual_seed(batch * 7 + m)
    a = torch.rand((batch, m, k), device="cuda", generator=g) - 0.5
    b = torch.rand((batch, k, n), device="cuda", generator=g) - 0.5
    c = torch.empty((batch, m, n), device="cuda")
    return a, b, c


def best_of(fns, bursts):
    for f in fns.values():
        f()
    ms = {name: [] for name in fns}
    for _ in range(bursts):
        for name, f in fns.items():
            ms[name].append(f())
    return {name: min(v) for name, v in ms.items()}


def event_ms(call, reps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def batched_ms(mm, batch, m, n, k, a, b, c, reps):
    import torch
    s = torch.cuda.current_stream().cuda_stream
    return mm.time_sgemm_batched(0, 0, m, n, k, a.data_ptr(), k, m * k, b.data_ptr(), n, k * n, c.data_ptr(), n, m * n, batch, 0,
                                 reps, s)


EX_SHAPES = [(512, 128), (64, 256), (64, 512), (64, 1024), (512, 512), (2, 4096)]   # batch x cube: profiles/batched_sweep.md's
EX_ALPHA, EX_BETA = 0.7, 0.5


def ex_variants(mm, batch, s, epilogue):
    """{"fused", "unfused", "plain"}: callables that enqueue one call each on torch's current stream."""
    import torch
    import how_to_optimize_gemm_amd as H
    a, b, c = operands(batch, s, s, s)
    g = torch.Generator(device="cuda").manual_seed(batch + s)
    c.copy_(torch.rand((batch, s, s), device="cuda", generator=g) - 0.5)
    bias = torch.rand((batch, s), device="cuda", generator=g) - 0.5
    tmp = torch.empty_like(c)
    st = torch.cuda.current_stream().cuda_stream
    pa, pb, pc, sz = a.data_ptr(), b.data_ptr(), c.data_ptr(), s * s
    if epilogue == "alpha_beta":
        def fused():
            mm.sgemm_batched_ex(0, 0, s, s, s, EX_ALPHA, pa, s, sz, pb, s, sz, EX_BETA, pc, s, sz, batch, 0, 0, H.BIAS_NONE, H.ACT_NONE, st)

        def unfused():   # c = beta c + alpha (a @ b): the product needs a buffer of its own
            mm.bmm(a, b, out=tmp)
            c.mul_(EX_BETA).add_(tmp, alpha=EX_ALPHA)
    else:
        def fused():
            mm.sgemm_batched_ex(0, 0, s, s, s, 1.0, pa, s, sz, pb, s, sz, 0.0, pc, s, sz, batch, bias.data_ptr(), s, H.BIAS_COL,
                                H.ACT_RELU, st)

        def unfused():
            mm.bmm(a, b, out=c)
            c.add_(bias[:, None, :]).relu_()

    def plain():
        mm.sgemm_batched(0, 0, s, s, s, pa, s, sz, pb, s, sz, pc, s, sz, batch, False, st)
    return {"fused": fused, "unfused": unfused, "plain": plain}, (a, b, c, bias, tmp)


def ex_sweep(args):
    import statistics
    import torch
    import how_to_optimize_gemm_amd as H
    mm = H.MMult(0, "auto")
    dev = mm.device_info()
    passes = max(3, args.passes)
    rows = []
    for batch, s in EX_SHAPES:
        for epilogue in ("alpha_beta", "bias_relu"):
            fns, keep = ex_variants(mm, batch, s, epilogue)
            reps = min(2000, max(5, int(8e12 / (2.0 * batch * s ** 3))))
            for f in fns.values():   # warm-up: every variant, as often as a timed window runs it
                event_ms(f, reps)
            fns["fused"]()
            torch.cuda.synchronize()
            launch = H.last_launch()
            ms = {name: [] for name in fns}
            for _ in range(passes):
                for name, f in fns.items():
                    ms[name].append(event_ms(f, reps))
            med = {name: statistics.median(v) for name, v in ms.items()}
            spread = {name: max(v) - min(v) for name, v in ms.items()}
            bias_mode, sbias = (H.BIAS_COL, s) if epilogue == "bias_relu" else (H.BIAS_NONE, 0)
            kernel, form, _ = H.auto_plan_batched_ex(0, 0, s, s, s, batch=batch, bias_mode=bias_mode, stride_bias=sbias,
                                                     cu_count=dev["cu_count"])
            row = {"shape": [batch, s, s, s], "epilogue": epilogue, "form": form, "kernel": kernel, "reps": reps, "launch": launch,
                   "ms": med, "spread_ms": spread, "not_slower": med["fused"] <= med["unfused"] + spread["unfused"]}
            rows.append(row)
            print(json.dumps(row), flush=True)
            del fns, keep
            torch.cuda.empty_cache()
    mm.close()
    us = lambda row, name: f"{1e3 * row['ms'][name]:.1f} +- {1e3 * row['spread_ms'][name]:.1f}"
    lines = ["# Batched SGEMM with the fused epilogue: one call against bmm + elementwise passes", "",
             f"Device: {dev['name']}, {dev['cu_count']} CUs.  Taken on {args.commit}.  `python tools/batched_sweep.py --ex`: microseconds "
             f"per call, device events around `reps` back-to-back calls after a warm-up window of the same length, median +- spread "
             f"(max - min) of {passes} passes with the three variants interleaved in every pass.  Operands packed row-major (fp32, NN), "
             "issued from Python on one stream.", "",
             f"- **fused**: one `mmh_sgemm_batched_ex` call on `MMH_KERNEL_AUTO` (alpha = {EX_ALPHA}, beta = {EX_BETA}; or a column bias "
             "per matrix and ReLU).",
             "- **unfused**: what a caller had before: `MMult.bmm` and torch's in-place elementwise passes for the same result "
             "(`bmm` into a second buffer, `c.mul_(beta).add_(tmp, alpha=alpha)`; or `bmm`, `c.add_(bias[:, None, :]).relu_()`).",
             "- **plain**: `mmh_sgemm_batched` alone -- the floor: the same product without any epilogue.",
             "- **verdict**: `ok` where fused <= unfused + unfused's own spread (the fusion must not lose to the sequence it replaces).",
             "",
             "| batch x m x n x k | epilogue | AUTO form (tile) | reps | fused us | unfused us | plain us | fused / unfused | fused / plain | verdict |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for row in rows:
        bt, m, n, k = row["shape"]
        lines.append(f"| {bt} x {m} x {n} x {k} | {row['epilogue']} | {row['form']} ({row['kernel']}) | {row['reps']} | {us(row, 'fused')} | "
                     f"{us(row, 'unfused')} | {us(row, 'plain')} | {row['ms']['fused'] / row['ms']['unfused']:.3f} | "
                     f"{row['ms']['fused'] / row['ms']['plain']:.3f} | {'ok' if row['not_slower'] else 'SLOWER'} |")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    open(args.out, "w").write("\n".join(lines) + "\n")
    print("wrote", args.out)
    return 0 if all(row["not_slower"] for row in rows) else 3


def raster_ab(bursts):
    import how_to_optimize_gemm_amd as H
    H.use_ab_library(build=False)
    mm = H.MMult(0, "auto")
    for batch, m, n, k in RASTER_SHAPES:
        a, b, c = operands(batch, m, n, k)
        reps = max(3, int(2e10 / (2 * batch * m * n * k)))

        def order(major):
            def f():
                mm.set_option(OPT_BATCH_MAJOR, major)
                return batched_ms(mm, batch, m, n, k, a, b, c, reps)
            return f
        best = best_of({"xcd_runs": order(0), "batch_major": order(1)}, bursts)
        mm.set_option(OPT_BATCH_MAJOR, 0)
        mm.time_sgemm_batched(0, 0, m, n, k, a.data_ptr(), k, m * k, b.data_ptr(), n, k * n, c.data_ptr(), n, m * n, batch, 0, 1, 0)
        print(json.dumps({"shape": [batch, m, n, k], "launch": H.last_launch(),
                          "xcd_runs": tflops(batch, m, n, k, best["xcd_runs"]),
                          "batch_major": tflops(batch, m, n, k, best["batch_major"])}), flush=True)
    mm.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--raster-ab", action="store_true")
    ap.add_argument("--quick", action="store_true", help="fewer bursts")
    ap.add_argument("--ex", action="store_true", help="the fused epilogue against bmm + elementwise passes")
    ap.add_argument("--passes", type=int, default=5, help="--ex: timed passes (at least 3)")
    ap.add_argument("--commit", default="an unnamed working tree", help="--ex: what the table says it was taken on")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(REPO, "profiles", "batched_ex_sweep.md" if args.ex else "batched_sweep.md")
    if args.ex:
        sys.exit(ex_sweep(args))
    bursts = 3 if args.quick else 5
    if args.raster_ab:
        raster_ab(bursts)
        return
    import torch
    import how_to_optimize_gemm_amd as H
    mm = H.MMult(0, "auto")
    dev = mm.device_info()
    rows = []
    for batch, m, n, k in SHAPES:
        a, b, c = operands(batch, m, n, k)
        reps = max(2, int(2e10 / (2 * batch * m * n * k)))
        s = torch.cuda.current_stream().cuda_stream

        def loop():
            def once():
                for i in range(batch):
                    mm.sgemm_op(0, 0, m, n, k, a[i].data_ptr(), k, b[i].data_ptr(), n, c[i].data_ptr(), n, False, s)
            return event_ms(once, reps)

        best = best_of({"auto": lambda: batched_ms(mm, batch, m, n, k, a, b, c, reps), "loop": loop,
                        "torch": lambda: event_ms(lambda: torch.bmm(a, b, out=c), reps)}, bursts)
        form, plan_kernel = H.auto_plan_batched(0, 0, m, n, k, batch=batch)[1], H.auto_plan_batched(0, 0, m, n, k, batch=batch)[0]
        row = {"shape": [batch, m, n, k], "form": form, "kernel": plan_kernel,
               **{key: tflops(batch, m, n, k, v) for key, v in best.items()}}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del a, b, c
        torch.cuda.empty_cache()
    mm.close()
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--raster-ab"] + (["--quick"] if args.quick else []),
                       capture_output=True, text=True, timeout=1200)
    raster = [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
    if r.returncode != 0:
        print(r.stdout[-2000:], r.stderr[-2000:])
    lines = ["# Strided batched SGEMM: AUTO against a loop of mmh_sgemm_op and torch.bmm", "",
             f"Device: {dev['name']}, {dev['cu_count']} CUs.  `python tools/batched_sweep.py`: TFLOP/s (2 batch m n k / time), "
             f"best of {bursts} interleaved bursts, operands packed row-major (fp32, NN).", "",
             "- **AUTO**: one `mmh_sgemm_batched` call (its form: fold, one launch of `sgemm_mfma_dma5_batched_kernel`, or a "
             "loop of the per-matrix plan).",
             "- **loop**: `batch` calls of `mmh_sgemm_op` from Python, one per matrix.",
             "- **torch.bmm**: the BLAS bundled in torch's wheel on the same tensors -- a different library from this one, "
             "not a build of it.", "",
             "| batch x m x n x k | AUTO form (tile) | AUTO | loop of mmh_sgemm_op | AUTO / loop | torch.bmm (bundled BLAS) | AUTO / torch.bmm |",
             "|---|---|---|---|---|---|---|"]
    for row in rows:
        bt, m, n, k = row["shape"]
        lines.append(f"| {bt} x {m} x {n} x {k} | {row['form']} ({row['kernel']}) | {row['auto']:.1f} | {row['loop']:.1f} | "
                     f"{row['auto'] / row['loop']:.2f} | {row['torch']:.1f} | {row['auto'] / row['torch']:.2f} |")
    lines += ["", "## Raster of the one-launch form", "",
              "The dispatcher deals a launch's workgroups round-robin over the 8 XCDs.  XCD-contiguous runs: the linear id is "
              "remapped so that each XCD takes a run of consecutive ids (a small matrix's tiles on one L2).  Batch-major: "
              "the plain order.  Tools build (`libmmult_hip_ab.so`, option 108), same process, interleaved bursts.", "",
              "| batch x m x n x k | launch | XCD-contiguous | batch-major | ratio |", "|---|---|---|---|---|"]
    for row in raster:
        bt, m, n, k = row["shape"]
        tile = row["launch"].split(" ")[0].replace("sgemm_mfma_dma5_batched_kernel", "")
        lines.append(f"| {bt} x {m} x {n} x {k} | {tile} | {row['xcd_runs']:.1f} | {row['batch_major']:.1f} | "
                     f"{row['xcd_runs'] / row['batch_major']:.3f} |")
    if not raster:
        lines.append("| (the tools build did not run: " + (r.stderr.strip().splitlines() or ["?"])[-1][:200] + ") | | | | |")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    open(args.out, "w").write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
