#!/usr/bin/env python3
"""linear_backward_sweep.py -- the linear layer's backward: what the gate + bias-gradient pass (mmh_relu_grad_colsum) costs,
alone and beside the two GEMMs.
(a) the primitive -- gate + dz + column sum -- at four shapes, timed by mmh_time_relu_grad_colsum (calls issued from C), in
    us and in GB/s counted as 3 rows cols 4 bytes (g and y read, dz written), beside mmh_probe_hbm_copy's rate from the same
    session and beside what it replaces, torch.where(y > 0, g, 0) then .sum(0) (events around the repetitions); also the
    column-sum-only and the gate-only modes;
(b) MMult.linear_backward (all three gradients, ReLU) at two layer shapes: its time, the pass's share of it, and torch
    autograd's backward of relu(F.linear(x, w, b)) -- the BLAS bundled in torch's wheel -- for the same gradients.
Every figure is the median of `--passes` interleaved passes.  Writes profiles/linear_backward_sweep.md.

    python tools/linear_backward_sweep.py [--passes 5] [--reps 20] [--out profiles/linear_backward_sweep.md]"""
import argparse
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import torch  # noqa: E402
import how_to_optimize_gemm_amd as H  # noqa: E402

PRIMITIVE = [(4096, 4096), (16384, 4096), (65536, 1024), (512, 512)]
LAYERS = [(4096, 4096, 4096), (8192, 1024, 4096)]   # (rows, in, out)


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


def medians(calls, passes, reps):
    """{name: median ms} of `passes` interleaved passes over calls = {name: fn(reps, warm)}."""
    for fn in calls.values():
        fn(3, 3)
    ms = {name: [] for name in calls}
    for _ in range(passes):
        for name, fn in calls.items():
            ms[name].append(fn(reps, 0))
    return {name: statistics.median(v) for name, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "linear_backward_sweep.md"))
    args = ap.parse_args()
    mm = H.MMult(0, "auto")
    hbm = mm.probe_hbm_copy()
    prim = []
    for rows, cols in PRIMITIVE:
        g = torch.randn((rows, cols), device="cuda")
        y = torch.randn((rows, cols), device="cuda")
        dz, s = torch.empty_like(g), torch.empty(cols, device="cuda")
        zero = torch.zeros((), device="cuda")
        calls = {
            "full": lambda reps, warm: mm.time_relu_grad_colsum(g, y, dz=dz, bias_grad=s, warmup=warm, reps=reps),
            "colsum": lambda reps, warm: mm.time_relu_grad_colsum(g, None, want_dz=False, bias_grad=s, warmup=warm, reps=reps),
            "gate": lambda reps, warm: mm.time_relu_grad_colsum(g, y, dz=dz, want_colsum=False, warmup=warm, reps=reps),
            "torch": lambda reps, warm: events(lambda: torch.where(y > 0, g, zero).sum(0), reps, warm),
        }
        med = medians(calls, args.passes, args.reps)
        mm.relu_grad_colsum(g, y, dz=dz, bias_grad=s)
        prim.append((rows, cols, med, H.last_launch()))
        print(rows, cols, " ".join(f"{k} {v * 1e3:.1f}us" for k, v in med.items()), flush=True)
        del g, y, dz
    layers = []
    for rows, n_in, n_out in LAYERS:
        x = torch.randn((rows, n_in), device="cuda")
        w = torch.randn((n_out, n_in), device="cuda") / n_in ** 0.5
        b = torch.randn(n_out, device="cuda")
        g = torch.randn((rows, n_out), device="cuda")
        y = mm.linear(x, w, b, "relu")
        dz, s = torch.empty_like(g), torch.empty(n_out, device="cuda")
        xt, wt, bt = (t.clone().requires_grad_(True) for t in (x, w, b))
        yt = torch.relu(torch.nn.functional.linear(xt, wt, bt))

        def torch_backward():
            torch.autograd.grad(yt, (xt, wt, bt), g, retain_graph=True)

        calls = {
            "ours": lambda reps, warm: events(lambda: mm.linear_backward(g, x, w, y), reps, warm),
            "pass": lambda reps, warm: mm.time_relu_grad_colsum(g, y, dz=dz, bias_grad=s, warmup=warm, reps=reps),
            "torch": lambda reps, warm: events(torch_backward, reps, warm),
        }
        med = medians(calls, args.passes, max(args.reps // 2, 1))
        layers.append((rows, n_in, n_out, med))
        print(rows, n_in, n_out, " ".join(f"{k} {v * 1e3:.1f}us" for k, v in med.items()), flush=True)
        del x, w, g, y, dz, xt, wt, yt
    dev = "MI355X" if "gfx950" in torch.cuda.get_device_properties(0).gcnArchName else torch.cuda.get_device_properties(0).name
    with open(args.out, "w") as fo:
        fo.write("# The linear layer's backward: the gate + bias-gradient pass, alone and beside the GEMMs\n\n")
        fo.write(f"`python tools/linear_backward_sweep.py --passes {args.passes} --reps {args.reps}` on one {dev}: the median of "
                 f"{args.passes} interleaved passes after a warm-up.  MMH_COLSUM_BLOCK_ROWS = {H.COLSUM_BLOCK_ROWS}.  "
                 f"mmh_probe_hbm_copy in the same session: {hbm:.0f} GB/s (read + write bytes).\n\n")
        fo.write("## (a) The primitive\n\n")
        fo.write("full = gate + dz + column sum (mmh_time_relu_grad_colsum), GB/s counted as 3 rows cols 4 bytes; colsum only = no "
                 "gate, no dz (1 pass); gate only = dz without the sum (3 passes); torch = `torch.where(y > 0, g, 0)` then `.sum(0)` "
                 "(4 passes), events around the repetitions.\n\n")
        fo.write("| rows | cols | full us | full GB/s | of the copy rate | colsum only us | GB/s (1 pass) | gate only us | GB/s (3 passes) | "
                 "torch us | torch / full |\n|---|---|---|---|---|---|---|---|---|---|---|\n")
        for rows, cols, med, _ in prim:
            one = rows * cols * 4 / 1e9
            gb = lambda passes, ms: passes * one / (ms * 1e-3)
            fo.write(f"| {rows} | {cols} | {med['full'] * 1e3:.1f} | {gb(3, med['full']):.0f} | {gb(3, med['full']) / hbm:.2f} | "
                     f"{med['colsum'] * 1e3:.1f} | {gb(1, med['colsum']):.0f} | {med['gate'] * 1e3:.1f} | {gb(3, med['gate']):.0f} | "
                     f"{med['torch'] * 1e3:.1f} | {med['torch'] / med['full']:.2f} |\n")
        fo.write("\nLaunches of the full form:\n\n")
        for rows, cols, _, launch in prim:
            fo.write(f"- {rows} x {cols}: `{launch}`\n")
        fo.write("\n## (b) linear_backward (dx, dw, db; ReLU)\n\n")
        fo.write("ours = MMult.linear_backward issued from Python (the pass, then mmh_sgemm and mmh_sgemm_op TN on MMH_KERNEL_AUTO); "
                 "pass = the pass alone; torch = torch.autograd.grad through relu(F.linear(x, w, b)) for the same three gradients, on "
                 "the BLAS bundled in torch's wheel.\n\n")
        fo.write("| rows | in | out | ours us | pass us | pass share | ours TFLOP/s (4 rows in out) | torch us | torch / ours |\n"
                 "|---|---|---|---|---|---|---|---|---|\n")
        for rows, n_in, n_out, med in layers:
            fo.write(f"| {rows} | {n_in} | {n_out} | {med['ours'] * 1e3:.1f} | {med['pass'] * 1e3:.1f} | "
                     f"{med['pass'] / med['ours']:.3f} | {4.0 * rows * n_in * n_out / (med['ours'] * 1e-3) / 1e12:.1f} | "
                     f"{med['torch'] * 1e3:.1f} | {med['torch'] / med['ours']:.2f} |\n")
    mm.close()
    print("wrote", args.out)


if __name__ == "__main__":
    main()
