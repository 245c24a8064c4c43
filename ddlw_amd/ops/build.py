"""Build the in-tree HIP kernel library for gfx950.

Usage: ``python -m ddlw_amd.ops.build`` (also called by ``__graft_entry__.build``).
Raw ``hipcc --offload-arch=gfx950`` — no hipify, no CUDA path. The resulting
``libddlw_kernels.so`` sits next to this file so it travels with repo
snapshots to GPU boxes (it is git-ignored; history stays source-only).
"""
from __future__ import annotations

import hashlib
import json
import os
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

HERE = Path(__file__).resolve().parent
HIP_DIR = HERE / "hip"
OUT = HERE / "libddlw_kernels.so"
STAMP = HERE / ".build_stamp.json"

SOURCES = sorted(HIP_DIR.glob("*.hip"))
HIPCC = "/opt/rocm/bin/hipcc"

FLAGS = [
    "--offload-arch=gfx950",
    "-O3",
    "-std=c++17",
    "-fPIC",
    "-shared",
    "-ffast-math",
    "-fvisibility=hidden",
]

# Files compiled without packed fp32 arithmetic (v_pk_add_f32, v_pk_mul_f32,
# v_pk_fma_f32) on top of FLAGS. A flag of the whole library would change the
# device code of every kernel in it, so it is per file: every source is
# compiled to an object of its own with its own flags, then linked.
NO_PK_F32 = ["-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops"]
FILE_FLAGS = {
    "bn_folded.hip": NO_PK_F32,
    "pointwise_deep.hip": NO_PK_F32,
    "weights.hip": NO_PK_F32,
}
# the host half of a compile does not know the device feature and says so
_NOISE = "'-packed-fp32-ops' is not a recognized feature for this target"


def compile_flags(src: Path) -> list:
    """Compiler flags of one source file, without the link step's -shared."""
    return [f for f in FLAGS if f != "-shared"] + FILE_FLAGS.get(src.name, [])


def _digest() -> str:
    h = hashlib.sha256()
    for f in SOURCES + sorted(HIP_DIR.glob("*.h")):
        h.update(f.name.encode())
        h.update(f.read_bytes())
    h.update(" ".join(FLAGS).encode())
    h.update(json.dumps(FILE_FLAGS, sort_keys=True).encode())
    return h.hexdigest()


def _run(cmd: list, verbose: bool) -> None:
    if verbose:
        print("[ddlw.ops.build]", " ".join(cmd), flush=True)
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        sys.stderr.write(res.stdout + res.stderr)
        raise RuntimeError(f"hipcc failed ({res.returncode})")
    warn = "".join(l for l in res.stderr.splitlines(True) if _NOISE not in l)
    if warn.strip() and verbose:
        sys.stderr.write(warn)


def build(force: bool = False, verbose: bool = True) -> Path:
    dig = _digest()
    if not force and OUT.exists() and STAMP.exists():
        try:
            if json.loads(STAMP.read_text()).get("digest") == dig:
                if verbose:
                    print(f"[ddlw.ops.build] up to date: {OUT}")
                return OUT
        except Exception:
            pass
    with tempfile.TemporaryDirectory(prefix="ddlw_build_") as tmp:
        objs = [str(Path(tmp) / (src.stem + ".o")) for src in SOURCES]
        with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
            list(pool.map(
                lambda so: _run([HIPCC, *compile_flags(so[0]), "-c", str(so[0]),
                                 "-o", so[1]], verbose),
                zip(SOURCES, objs)))
        _run([HIPCC, "-shared", "-fPIC", *objs, "-o", str(OUT)], verbose)
    STAMP.write_text(json.dumps({"digest": dig}))
    if verbose:
        print(f"[ddlw.ops.build] built {OUT}")
    return OUT


if __name__ == "__main__":
    build(force="--force" in sys.argv)
