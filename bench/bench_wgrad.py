#!/usr/bin/env python3
"""3x3 stride-1 weight-gradient microbenchmark: the tap-fused kernel
(``k_conv_wgrad3x3``) vs the per-tap kernel (``k_conv_wgrad``) vs the library
(``torch.nn.grad.conv2d_weight``, MIOpen).

For each of ResNet-50's four stride-1 3x3 layers at ``--batch`` images:
  1. parity-check both ddlw kernels against the fp32 reference (first 4
     images);
  2. time the three contenders in alternating rounds inside this one process
     (device events around ``--iters`` back-to-back calls; median and
     spread = max - min over ``--rounds`` rounds);
  3. print one JSON line per shape. ``route_taps`` applies the routing rule:
     the tap-fused kernel is the default only where its median beats the
     per-tap kernel's median by more than the per-tap kernel's spread.

Run on an MI355X:  python bench/bench_wgrad.py [--batch 256] [--no-taps]
``--no-taps`` leaves the new kernel out (per-shape times of the per-tap
kernel alone).
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from ddlw_amd.ops import conv_gemm  # noqa: E402

# (H = W, C = K): ResNet-50's stride-1 3x3 convs at 224 input
RESNET50_3X3_S1 = [(56, 64), (28, 128), (14, 256), (7, 512)]


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _round_ms(fn, iters: int) -> float:
    start = torch.cuda.Event(enable_timing=True)
    stop = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def time_interleaved(fns: dict, iters: int, rounds: int, warmup: int = 3) -> dict:
    """{name: (median_ms, spread_ms)}; the contenders alternate round by round."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            samples[k].append(_round_ms(fn, iters))
    return {k: (statistics.median(v), max(v) - min(v)) for k, v in samples.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--no-taps", action="store_true")
    ap.add_argument("--out", type=str, default="bench_out/wgrad_report.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_wgrad: no GPU (timings are only meaningful on the device)")
    dev = torch.device("cuda:0")
    B = args.batch
    report = []
    for (H, C) in RESNET50_3X3_S1:
        K, wshape = C, (C, C, 3, 3)
        torch.manual_seed(0)
        x = _cl(torch.randn(B, C, H, H, device=dev).to(torch.bfloat16))
        dy = _cl(torch.randn(B, K, H, H, device=dev).to(torch.bfloat16))

        def taps():
            return conv_gemm.conv_wgrad3x3_kernel(dy, x, wshape, 1, 1)

        def pertap():
            return conv_gemm.conv_wgrad_pertap_kernel(dy, x, wshape, 1, 1)

        def lib():
            return torch.nn.grad.conv2d_weight(x, wshape, dy, stride=1, padding=1)

        xs, dys = _cl(x[:4]), _cl(dy[:4])
        ref = torch.nn.grad.conv2d_weight(xs.float(), wshape, dys.float(),
                                          stride=1, padding=1)
        scale = ref.abs().max() + 1e-6
        rec = {"shape": f"n{B}_h{H}_c{C}_k{K}_3x3s1"}
        fns = {"pertap": pertap, "lib": lib}
        e_old = ((conv_gemm.conv_wgrad_pertap_kernel(dys, xs, wshape, 1, 1).float()
                  - ref).abs().max() / scale).item()
        rec["err_pertap"] = round(e_old, 5)
        if not args.no_taps:
            fns = {"taps": taps, **fns}
            e_new = ((conv_gemm.conv_wgrad3x3_kernel(dys, xs, wshape, 1, 1).float()
                      - ref).abs().max() / scale).item()
            rec["err_taps"] = round(e_new, 5)
            rec["parity_ok"] = e_new <= 5e-2 and e_new <= 2 * e_old + 1e-3

        t = time_interleaved(fns, args.iters, args.rounds)
        flop = 2.0 * B * H * H * K * C * 9
        for k, (med, spread) in t.items():
            rec[f"us_{k}"] = round(med * 1e3, 1)
            rec[f"spread_us_{k}"] = round(spread * 1e3, 1)
            rec[f"tflops_{k}"] = round(flop / med / 1e9, 1)
        if not args.no_taps:
            rec["route_taps"] = t["taps"][0] < t["pertap"][0] - t["pertap"][1]
            rec["taps_beats_lib"] = t["taps"][0] < t["lib"][0] - t["lib"][1]
        report.append(rec)
        print(json.dumps(rec), flush=True)

    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(report, indent=2))


if __name__ == "__main__":
    main()
