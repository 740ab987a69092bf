"""tools/trace_write_rate.py in its small form (-m gpu): it runs as a child process on a 2 x 128 network and 8 games, compares the
device writer's texts with the host writer's before it times anything (it exits non-zero otherwise), and every timing and rate
of its line is finite and positive; the file holds what was printed."""
import json
import math
import os
import subprocess
import sys

import pytest

from support import ROOT

ROWS = ("host", "device", "device_files")


@pytest.mark.gpu
def test_small_form_runs(tmp_path):
    out = tmp_path / "lines.jsonl"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "trace_write_rate.py"), "--reps", "2", "--games", "8", "--blocks", "2",
                        "--channels", "128", "--out", str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-2000:]
    print(r.stdout)
    lines = [json.loads(ln) for ln in r.stdout.splitlines()]
    assert len(lines) == 1 and out.read_text() == r.stdout
    x = lines[0]
    assert x["tool"] == "trace_write_rate" and x["games"] == 8 and x["plies"] > 0 and x["children"] > 0
    assert x["text_bytes"] > 80 * x["children"] and sorted(x["rows"]) == sorted(ROWS)
    timings = [x["host_over_device"]] + [x["rows"][r][k] for r in ROWS for k in ("call_ms", "call_ms_min", "call_ms_max", "text_MB_per_s", "games_per_s")]
    timings += [x["rows"]["device"][k] for k in ("count_ms", "emit_ms", "emit_text_GB_per_s", "hbm_frac")]
    assert all(isinstance(v, (int, float)) and math.isfinite(v) and v > 0 for v in timings), timings
    for r in ROWS:
        assert x["rows"][r]["call_ms_min"] <= x["rows"][r]["call_ms"] <= x["rows"][r]["call_ms_max"]
