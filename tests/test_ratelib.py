"""tools/ratelib.py without a device: the statistics, the record and its writer, the protocol of the event-timed loop against a
stub runtime that logs its calls (the loop the files in profiles/ were made with), and every rate tool's --help."""
import json
import os
import re
import subprocess
import sys

import pytest

import ratelib
from support import ROOT, scamd_built  # noqa: F401

TOOLS = ("encode_device_rate", "san_rate", "san_write_rate", "score_rate", "merge_rate", "train_batch_rate", "fen_rate", "perft_rate",
         "match_time")


@pytest.fixture(autouse=True)
def no_runtime(monkeypatch):
    def refuse():
        raise AssertionError("hip_runtime() called in a test without a device")
    monkeypatch.setattr(ratelib.scamd, "hip_runtime", refuse)


def test_spread_odd_and_even():
    assert ratelib.spread([3.0, 1.0, 2.0]) == (2.0, 1.0, 3.0)
    assert ratelib.spread([4.0, 1.0, 3.0, 2.0]) == (2.5, 1.0, 4.0)
    assert ratelib.spread([7.0]) == (7.0, 7.0, 7.0)


def test_record_starts_with_tool_host_date():
    r = ratelib.record("some_rate", plies=5, rows={"a": 1})
    assert list(r)[:3] == ["tool", "host", "date"] and r["tool"] == "some_rate"
    assert list(r)[3:] == ["plies", "rows"] and r["plies"] == 5
    assert r["host"] and len(r["date"]) == 10


def test_emit_appends_creates_and_skips_devnull(tmp_path, capsys, monkeypatch):
    lines = [{"tool": "t", "a": 1}, {"tool": "t", "a": 2}]
    text = "".join(json.dumps(ln) + "\n" for ln in lines)
    f = tmp_path / "there.jsonl"
    f.write_text("old\n")
    ratelib.emit(lines, str(f), "t")
    assert f.read_text() == "old\n" + text and capsys.readouterr().out == text
    g = tmp_path / "new" / "dir" / "x.jsonl"
    ratelib.emit(lines, str(g), "t")
    assert g.read_text() == text and capsys.readouterr().out == text
    ratelib.emit(lines, str(f), "t", mode="w")
    assert f.read_text() == text and capsys.readouterr().out == text
    # os.devnull: printed, nothing written (a default file would land under ROOT/profiles)
    monkeypatch.setattr(ratelib, "ROOT", str(tmp_path / "root"))
    ratelib.emit(lines, os.devnull, "t")
    assert capsys.readouterr().out == text and not (tmp_path / "root").exists()
    ratelib.emit(lines, None, "t")
    made = list((tmp_path / "root" / "profiles").iterdir())
    assert len(made) == 1 and made[0].name.startswith("t_") and made[0].name.endswith(".jsonl") and made[0].read_text() == text
    assert capsys.readouterr().out == text


class StubHip:
    """the runtime calls Hip makes, logged by name"""

    def __init__(self):
        self.log = []

    def __getattr__(self, name):
        def fn(*args):
            self.log.append(name)
            if name == "hipEventElapsedTime":
                args[0]._obj.value = 0.25
            elif name in ("hipStreamCreate", "hipEventCreate", "hipMalloc"):
                args[0]._obj.value = 0x1000 + len(self.log)
            return 0
        return fn


class StubLib:
    def sc_last_error(self):
        return b"the stub's error"


def test_hip_timed_protocol():
    hip = StubHip()
    h = ratelib.Hip(StubLib(), hip)
    assert hip.log == ["hipStreamCreate", "hipEventCreate", "hipEventCreate"]
    events = []
    del hip.log[:]

    def call():
        hip.log.append("call")
        return 0
    hip_record = hip.hipEventRecord

    def record(e, s):   # which event, on which stream
        events.append((e.value, s.value))
        return hip_record(e, s)
    hip.hipEventRecord = record
    reps = 3
    call_ms, enqueue_ms, device_ms = h.timed(call, reps)
    region = ["hipEventRecord", "call", "hipEventRecord", "hipStreamSynchronize", "hipEventElapsedTime"]
    assert hip.log == ["call", "hipStreamSynchronize"] + region * reps
    assert events == [(h.e0.value, h.stream.value), (h.e1.value, h.stream.value)] * reps and h.e0.value != h.e1.value
    assert len(call_ms) == len(enqueue_ms) == len(device_ms) == reps
    assert device_ms == [0.25] * reps and all(0 <= e <= c for e, c in zip(enqueue_ms, call_ms))
    q = h.alloc(16)
    del hip.log[:]
    h.close()
    assert hip.log == ["hipFree", "hipEventDestroy", "hipEventDestroy", "hipStreamDestroy"] and q.value and h.bufs == []


def test_hip_timed_raises_on_a_return_code():
    hip = StubHip()
    h = ratelib.Hip(StubLib(), hip)
    with pytest.raises(AssertionError, match="the stub's error"):
        h.timed(lambda: 3, 2)
    codes = iter([0, 0, 3])
    del hip.log[:]
    with pytest.raises(AssertionError, match="the stub's error"):
        h.timed(lambda: next(codes), 5)   # the warm-up and one region pass, the second region's call fails
    assert hip.log.count("hipEventElapsedTime") == 1


@pytest.mark.parametrize("tool", TOOLS)
def test_tool_keeps_no_copy_of_the_shared_pieces(tool):
    with open(os.path.join(ROOT, "tools", tool + ".py")) as f:
        src = f.read()
    if tool == "perft_rate":   # the argument types of its own libsc_rules_host.so stay
        src = re.sub(r"H\.sct_\w+\.argtypes = .*", "", src)
    for pattern in (r"\.argtypes\s*=\s*\[C\.", r"def timed", r"socket\.gethostname", r"hipEventRecord"):
        assert not re.search(pattern, src), pattern
    for other in TOOLS:   # no tool imports another tool
        assert not re.search(r"^\s*(from|import)\s+%s\b" % other, src, re.M), other


@pytest.mark.parametrize("tool", TOOLS)
def test_tool_help_needs_no_device(tool, scamd):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", tool + ".py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--out" in r.stdout and "no HIP device" not in r.stdout + r.stderr
