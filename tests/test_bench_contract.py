"""The driver depends on bench.py's exact contract: single JSON line with the
required keys, N=1 default, finishes quickly. Validate on CPU."""
import json
import os
import subprocess
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent


def test_bench_json_contract(tmp_path):
    env = dict(os.environ)
    env["DDLW_HOME"] = str(tmp_path)
    res = subprocess.run(
        [sys.executable, str(REPO / "bench.py"), "--steps", "2", "--warmup", "1"],
        capture_output=True, text=True, timeout=900, env=env, cwd=str(REPO),
    )
    assert res.returncode == 0, res.stderr
    line = res.stdout.strip().splitlines()[-1]
    out = json.loads(line)
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup",
                "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                "dtype", "data", "config"):
        assert key in out, key
    assert out["n_gpus"] == 1
    assert out["steps"] == 2 and out["warmup"] == 1
    assert out["scaling"] == "weak"
    assert out["higher_is_better"] is True
    assert "global_batch" in out["config"] and "parallelism" in out["config"]


def test_bench_full_and_dump_outputs(tmp_path):
    """--full is accepted and --dump-outputs writes the last step's results
    as float32 .npy files (finite, within the 64 MB budget)."""
    import numpy as np

    env = dict(os.environ)
    env["DDLW_HOME"] = str(tmp_path)
    dump = tmp_path / "dump"
    res = subprocess.run(
        [sys.executable, str(REPO / "bench.py"), "--gpus", "1", "--steps", "1",
         "--warmup", "0", "--full", "--dump-outputs", str(dump)],
        capture_output=True, text=True, timeout=900, env=env, cwd=str(REPO),
    )
    assert res.returncode == 0, res.stderr
    out = json.loads(res.stdout.strip().splitlines()[-1])
    assert out["steps"] == 1 and out["warmup"] == 0
    assert out["ms_per_step"] > 0
    # ms_per_step and the headline value describe the same timed window
    imgs_per_step = out["config"]["global_batch"]
    assert abs(out["value"] - imgs_per_step / out["ms_per_step"] * 1000) <= 0.01 * out["value"]
    files = sorted(p.name for p in dump.iterdir())
    assert files == ["bn_running_stats.npy", "logits.npy", "loss.npy", "params.npy"]
    total = 0
    for name in files:
        a = np.load(dump / name)
        assert a.dtype == np.float32 and a.size > 0, name
        assert np.isfinite(a).all(), name
        total += a.nbytes
    assert total <= 64 * 1000 * 1000
    assert np.load(dump / "logits.npy").shape == (out["config"]["per_gpu_batch"], 1000)


def test_conv_dispatch_table_schema():
    """The measured router table must stay well-formed: every entry maps
    fwd/dgrad/wgrad to 'hip' or 'stock' (a corrupted table would silently
    route everything to the library)."""
    import json
    from pathlib import Path

    table = json.loads(
        (REPO / "ddlw_amd" / "ops" / "conv_dispatch.json").read_text())
    assert len(table) >= 20  # the 22 ResNet-50 body shapes
    for key, ent in table.items():
        assert set(ent) == {"fwd", "dgrad", "wgrad"}, key
        assert all(v in ("hip", "stock") for v in ent.values()), key
    # fwd must be fully hip (measured winner on all 22 routes)
    assert all(e["fwd"] == "hip" for e in table.values())
