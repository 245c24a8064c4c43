#!/usr/bin/env python3
"""Residual-join dgrad microbenchmark: the bounce epilogue with prefetched
side reads (the ``PF`` instantiations of ``k_conv_fwd_igemm``,
``DDLW_EPI_PREFETCH`` unset / 1) vs the in-order epilogue
(``DDLW_EPI_PREFETCH=0``).

The five conv1 dgrads of ResNet-50 at ``--batch`` images that carry the
residual join (``acc``, ``acc_mask``) and the previous block's bn3 reduce
(``bnb``) in their epilogue, through ``conv_gemm.conv_dgrad_kernel`` (so
each call includes the three tiny weight flip/transpose kernels, the same
for every contender):
  1. check that both levers give the same bits (dx and the partials);
  2. time the contenders in alternating rounds inside this one process
     (device events around ``--iters`` back-to-back calls; median and
     spread = max - min over ``--rounds`` rounds);
  3. print one JSON line per shape: us, achieved GB/s over the bytes the
     launch must move (dx write, acc read, bnb x read, the masks, dy) and
     TF/s. ``route_prefetch`` applies the routing rule: the new path is the
     default only where its median beats the old median by more than the old
     path's spread.

Run on an MI355X:  python bench/bench_join_dgrad.py [--batch 256]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from bench_wgrad import _cl, time_interleaved  # noqa: E402
from ddlw_amd.ops import conv_gemm  # noqa: E402

# (name, H = W, dy channels, dx channels, masked acc)
JOIN_DGRADS = [
    ("layer1_identity", 56, 64, 256, True),
    ("layer2_identity", 28, 128, 512, True),
    ("layer3_identity", 14, 256, 1024, True),
    ("layer4_identity", 7, 512, 2048, True),
    ("layer4_downsample_conv1", 14, 512, 1024, False),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", type=str, default="bench_out/join_dgrad_report.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_join_dgrad: no GPU (timings are only meaningful on the device)")
    dev = torch.device("cuda:0")
    B = args.batch
    report = []
    for (name, H, kdy, cdx, masked) in JOIN_DGRADS:
        torch.manual_seed(0)
        shape = (B, cdx, H, H)
        M = B * H * H
        w = _cl((torch.randn(kdy, cdx, 1, 1, device=dev) * 0.1).to(torch.bfloat16))
        dy = _cl(torch.randn(B, kdy, H, H, device=dev).to(torch.bfloat16))
        a = _cl(torch.randn(*shape, device=dev).to(torch.bfloat16))
        x_bn = _cl(torch.randn(*shape, device=dev).to(torch.bfloat16))
        mean = torch.randn(cdx, device=dev)
        rstd = torch.rand(cdx, device=dev) + 0.5
        m1 = (torch.randint(0, 256, (M * cdx // 8,), dtype=torch.uint8, device=dev)
              if masked else None)
        m2 = torch.randint(0, 256, (M * cdx // 8,), dtype=torch.uint8, device=dev)

        def call(lever):
            def fn():
                os.environ["DDLW_EPI_PREFETCH"] = lever
                return conv_gemm.conv_dgrad_kernel(
                    dy, w, shape, 0, 1, acc=a, acc_mask=m1,
                    bnb=(x_bn, m2, mean, rstd))
            return fn

        T = kdy // 64
        fns = {"inorder": call("0"), "prefetch": call("1")}
        outs = {k: fn() for k, fn in fns.items()}
        torch.cuda.synchronize()
        rec = {"shape": f"{name}_n{B}_h{H}_{kdy}to{cdx}", "T": T,
               "bit_equal": all(
                   torch.equal(o[0], outs["inorder"][0])
                   and torch.equal(o[1], outs["inorder"][1])
                   for o in outs.values())}
        del outs

        t = time_interleaved(fns, args.iters, args.rounds)
        nbytes = M * cdx * 2 * 3 + M * cdx // 8 * (2 if masked else 1) + M * kdy * 2
        flop = 2.0 * M * kdy * cdx
        rec["gbytes"] = round(nbytes / 1e9, 3)
        for k, (med, spread) in t.items():
            rec[f"us_{k}"] = round(med * 1e3, 1)
            rec[f"spread_us_{k}"] = round(spread * 1e3, 1)
            rec[f"gbps_{k}"] = round(nbytes / med / 1e6, 0)
            rec[f"tflops_{k}"] = round(flop / med / 1e9, 1)
        old_med, old_spread = t["inorder"]
        rec["route_prefetch"] = t["prefetch"][0] < old_med - old_spread
        report.append(rec)
        print(json.dumps(rec), flush=True)
        del w, dy, a, x_bn, m1, m2
        torch.cuda.empty_cache()

    os.environ.pop("DDLW_EPI_PREFETCH", None)
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(report, indent=2))


if __name__ == "__main__":
    main()
