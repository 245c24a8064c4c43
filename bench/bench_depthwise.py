#!/usr/bin/env python3
"""Depthwise 3x3 backward microbenchmark: ddlw dgrad/wgrad kernels vs the
library (``aten.convolution_backward``, MIOpen grouped conv).

For every distinct depthwise layer shape of MobileNetV2 @224:
  1. parity-check both kernels against the fp32 stock gradients;
  2. time kernel and library in alternating rounds inside this one process
     (device events around ``--iters`` back-to-back calls; median and min
     over ``--rounds`` rounds);
  3. print one JSON line per shape. ``gbps_*`` is the algorithmic traffic
     (each tensor read or written once) over the median time.

Run on an MI355X:  python bench/bench_depthwise.py [--batch 64]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from ddlw_amd.ops import binding  # noqa: E402

# (H = W, C, stride) — distinct depthwise layers of MobileNetV2 at 224 input
MOBILENET_V2_DW_SHAPES = [
    (112, 32, 1),
    (112, 96, 2),
    (56, 144, 1),
    (56, 144, 2),
    (28, 192, 1),
    (28, 192, 2),
    (14, 384, 1),
    (14, 576, 1),
    (14, 576, 2),
    (7, 960, 1),
]


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
    """{name: (median_ms, min_ms)}; the variants alternate round by round."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            samples[k].append(_round_ms(fn, iters))
    return {k: (statistics.median(v), min(v)) for k, v in samples.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", type=str, default="bench_out/depthwise_report.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_depthwise: no GPU (timings are only meaningful on the device)")
    dev = torch.device("cuda:0")
    B, pad = args.batch, 1
    report = []
    for (H, C, st) in MOBILENET_V2_DW_SHAPES:
        Ho = (H + 2 * pad - 3) // st + 1
        torch.manual_seed(0)
        x = _cl(torch.randn(B, C, H, H, device=dev).to(torch.bfloat16))
        w = torch.randn(C, 1, 3, 3, device=dev).to(torch.bfloat16)
        dy = _cl(torch.randn(B, C, Ho, Ho, device=dev).to(torch.bfloat16))

        def lib(mask):
            return torch.ops.aten.convolution_backward(
                dy, x, w, None, [st, st], [pad, pad], [1, 1], False, [0, 0], C, mask)

        # ---------- parity (first 4 images, fp32 reference) ----------
        xs, dys = _cl(x[:4]), _cl(dy[:4])
        ref_dx = torch.nn.grad.conv2d_input(
            xs.shape, w.float(), dys.float(), stride=st, padding=pad, groups=C)
        ref_dw = torch.nn.grad.conv2d_weight(
            xs.float(), w.shape, dys.float(), stride=st, padding=pad, groups=C)
        dx = binding.depthwise_dgrad(dys, w, tuple(xs.shape), st, pad).float()
        dw = binding.depthwise_wgrad(dys, xs, tuple(w.shape), st, pad)
        derr = ((dx - ref_dx).abs().max() / (ref_dx.abs().max() + 1e-6)).item()
        werr = ((dw - ref_dw).abs().max() / (ref_dw.abs().max() + 1e-6)).item()

        # ---------- timing ----------
        t = time_interleaved(
            {
                "hip_dgrad": lambda: binding.depthwise_dgrad(dy, w, tuple(x.shape), st, pad),
                "lib_dgrad": lambda: lib([True, False, False])[0],
                "hip_wgrad": lambda: binding.depthwise_wgrad(dy, x, tuple(w.shape), st, pad),
                "lib_wgrad": lambda: lib([False, True, False])[1],
            },
            args.iters, args.rounds,
        )
        bytes_io = 2.0 * (x.numel() + dy.numel())  # dgrad: dy in, dx out; wgrad: dy, x in
        rec = {
            "shape": f"n{B}_h{H}_c{C}_s{st}",
            "dgrad_err": round(derr, 5),
            "wgrad_err": round(werr, 5),
            "parity_ok": derr < 5e-2 and werr < 5e-2,
        }
        for k, (med, mn) in t.items():
            rec[f"ms_{k}"] = round(med, 4)
            rec[f"ms_min_{k}"] = round(mn, 4)
        rec["gbps_hip_dgrad"] = round(bytes_io / t["hip_dgrad"][0] / 1e6, 1)
        rec["gbps_hip_wgrad"] = round(bytes_io / t["hip_wgrad"][0] / 1e6, 1)
        rec["speedup_dgrad"] = round(t["lib_dgrad"][0] / t["hip_dgrad"][0], 2)
        rec["speedup_wgrad"] = round(t["lib_wgrad"][0] / t["hip_wgrad"][0], 2)
        report.append(rec)
        print(json.dumps(rec), flush=True)

    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(report, indent=2))


if __name__ == "__main__":
    main()
