"""The side-stream case table against the header (CPU): every entry of include/rtx.h with a
`void* hip_stream` parameter has a case in tests/test_stream_order_gpu.py, and its rtx.py wrapper takes a `stream`.
A new stream-taking entry without a side-stream case fails here."""
import inspect
import os
import re

import rtx
import stream_order as so
import test_stream_order_gpu as gpu_cases

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rtx.h")


def stream_entries():
    """The names of the prototypes of rtx.h that have a `void* hip_stream` parameter."""
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)  # comments
    text = re.sub(r"^\s*#.*$", " ", text, flags=re.M)  # preprocessor lines
    protos = re.findall(r"\b(rtx_\w+)\s*\(([^()]*)\)\s*;", text)
    assert len(protos) > 60, len(protos)
    return {name for name, params in protos if re.search(r"\bvoid\s*\*\s*hip_stream\b", params)}


def test_every_stream_taking_entry_has_a_side_stream_case():
    entries = stream_entries()
    assert len(entries) == 16, sorted(entries)
    assert entries == set(gpu_cases.CASES), (sorted(entries - set(gpu_cases.CASES)), sorted(set(gpu_cases.CASES) - entries))
    assert all(variants for _, variants in gpu_cases.CASES.values())
    assert len(set(gpu_cases.CASE_IDS)) == len(gpu_cases.CASE_IDS)


def test_every_wrapper_takes_a_stream():
    for entry, (wrapper, _) in gpu_cases.CASES.items():
        obj = rtx
        for part in wrapper.split("."):
            obj = getattr(obj, part)
        assert "stream" in inspect.signature(obj).parameters, (entry, wrapper)
        assert entry in inspect.getsource(obj), f"{wrapper} does not call {entry}"


def test_gate_length_rule():
    """20 times the slowest enqueue-only call's host time, at least 5 ms, at most 50 ms."""
    assert so.gate_target_ms(0.0) == 5.0
    assert so.gate_target_ms(100e-6) == 5.0
    assert abs(so.gate_target_ms(400e-6) - 8.0) < 1e-9
    assert so.gate_target_ms(10e-3) == 50.0
