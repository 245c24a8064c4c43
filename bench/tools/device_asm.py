#!/usr/bin/env python3
"""Per-kernel fingerprint of the emitted gfx950 device code.

Compiles every ``ddlw_amd/ops/hip/*.hip`` to device-only assembly with the
library's build flags and prints one ``file kernel sha256`` line per kernel
(function text + its ``.amdhsa_kernel`` descriptor). Host-side refactors must
leave the listing unchanged: run it on both trees and ``diff`` the outputs.

Usage: ``python bench/tools/device_asm.py [REPO_ROOT]`` (default: this tree).
"""
import hashlib
import re
import subprocess
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent.parent))
from ddlw_amd.ops.build import FLAGS, HIPCC  # noqa: E402


def kernels(asm: str) -> dict:
    """{symbol: text} — body and descriptor of each kernel. ``__hip_cuid_``
    lines differ between two compiles of the same file; the function index in
    local labels (.LBB<n>_, .Lfunc_end<n>) moves with instantiation order,
    and with its digit count the padding in front of a label's comment."""
    asm = "\n".join(l for l in asm.splitlines() if "__hip_cuid_" not in l)
    asm = re.sub(r"(\.LBB|\bBB|\.Lfunc_end|\.Lfunc_begin)\d+", r"\1", asm)
    asm = re.sub(r"[ \t]+;", " ;", asm)
    out = {}
    for m in re.finditer(r"^\t\.amdhsa_kernel (\S+)\n.*?^\t\.end_amdhsa_kernel$",
                         asm, re.M | re.S):
        sym = m.group(1)
        body = re.search(rf"^{re.escape(sym)}:.*?^\.Lfunc_end:$", asm, re.M | re.S)
        if body is None:
            raise SystemExit(f"no function body for kernel {sym}")
        out[sym] = body.group(0) + "\n" + m.group(0)
    return out


def main() -> int:
    root = Path(sys.argv[1] if len(sys.argv) > 1 else Path(__file__).parents[2])
    flags = [f for f in FLAGS if f != "-shared"]
    total = 0
    for src in sorted((root / "ddlw_amd" / "ops" / "hip").glob("*.hip")):
        res = subprocess.run([HIPCC, *flags, "--offload-device-only", "-S",
                              str(src), "-o", "-"], capture_output=True, text=True)
        if res.returncode != 0:
            sys.stderr.write(res.stderr)
            return 1
        for sym, text in sorted(kernels(res.stdout).items()):
            print(src.name, sym, hashlib.sha256(text.encode()).hexdigest())
            total += 1
    print(f"# {total} kernels", file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
