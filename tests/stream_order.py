"""Side-stream ordering checks for the entries of include/rtx.h that take a `void* hip_stream` — TEST
INFRASTRUCTURE, imported by test_stream_order_gpu.py.

Every other GPU test passes stream 0.  The legacy null stream waits for, and is waited for by, every blocking stream,
so on stream 0 a launch on the wrong stream, a missing event wait or a host memset nobody waits for computes the right
bytes.  Here nothing but stream order holds the calls together:

  side_stream   a NON-BLOCKING stream (torch's pool streams are; the flag is read back from the HIP runtime and
                asserted: on a blocking stream every check below would be vacuous)
  Gate          a finite delay of public torch ops (in-place adds on one large tensor) enqueued on a side stream,
                followed by a recorded event; its length is calibrated with events, not guessed
  run_on_side_stream
                the recipe: the real inputs arrive in the input buffers only BEHIND the gate, the outputs are poisoned
                again behind the gate, the call follows, the outputs are cloned on the stream.  A stage of the call
                that ran on any other stream read poisoned inputs, or had its output overwritten by the late poison,
                or was cloned before it finished: the bytes differ from the stream-0 bytes.  The gate's event, read
                straight after the call returns, says whether the call waited for the device.

No sleep intrinsic, no hand-written kernel, no spinning on host memory: a gate cannot wait for ever, and no two
streams ever wait for each other."""
from __future__ import annotations

import ctypes
import math
import time

import rtx

HIP_STREAM_NON_BLOCKING = 1  # hipStreamNonBlocking
POISON = 0xFF
GATE_FLOATS = 1 << 26  # 256 MiB: one in-place add moves 512 MiB, far longer on the device than its launch on the host
GATE_MIN_MS, GATE_MAX_MS, GATE_HOST_FACTOR = 5.0, 50.0, 20.0
GATE_MARGIN = 2.0  # the gates are made this many times the rule's minimum (up to the cap): host jitter on a shared machine

_owned = []  # streams made here with hipStreamCreateWithFlags (destroy_streams)


def hip():
    """The HIP runtime the process already runs on: librtx.so's handle resolves the runtime's symbols through its
    dependencies (one runtime per process, rtx.load)."""
    L = rtx.load()
    L.hipStreamGetFlags.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint)]
    L.hipStreamGetFlags.restype = ctypes.c_int
    L.hipStreamCreateWithFlags.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint]
    L.hipStreamCreateWithFlags.restype = ctypes.c_int
    L.hipStreamDestroy.argtypes = [ctypes.c_void_p]
    L.hipStreamDestroy.restype = ctypes.c_int
    return L


def stream_flags(stream) -> int:
    flags = ctypes.c_uint(0xFFFFFFFF)
    rc = hip().hipStreamGetFlags(ctypes.c_void_p(stream.cuda_stream), ctypes.byref(flags))
    assert rc == 0, f"hipStreamGetFlags: {rc}"
    return int(flags.value)


def side_stream(torch):
    """A non-blocking stream: torch's, or one made with hipStreamCreateWithFlags and wrapped."""
    s = torch.cuda.Stream()
    if stream_flags(s) != HIP_STREAM_NON_BLOCKING:
        h = ctypes.c_void_p()
        rc = hip().hipStreamCreateWithFlags(ctypes.byref(h), HIP_STREAM_NON_BLOCKING)
        assert rc == 0 and h.value, f"hipStreamCreateWithFlags: {rc}"
        _owned.append(h.value)
        s = torch.cuda.ExternalStream(h.value)
    assert s.cuda_stream != 0
    assert stream_flags(s) == HIP_STREAM_NON_BLOCKING, "a blocking side stream would make every check vacuous"
    return s


def destroy_streams(torch) -> None:
    torch.cuda.synchronize()
    while _owned:
        hip().hipStreamDestroy(ctypes.c_void_p(_owned.pop()))


def gate_target_ms(host_call_s: float) -> float:
    """The gate's length for a slowest enqueue-only call of host_call_s seconds: 20 times it, at least 5 ms, at most
    50 ms (so that every test stays within a few seconds)."""
    return min(GATE_MAX_MS, max(GATE_MIN_MS, GATE_HOST_FACTOR * host_call_s * 1e3))


class Gate:
    """`reps` in-place adds on a tensor of its own, then an event.  One Gate per side stream."""

    def __init__(self, torch, reps: int = 1):
        self.torch, self.reps = torch, reps
        self.t = torch.zeros(GATE_FLOATS, dtype=torch.float32, device="cuda")
        self.ms_per_rep = self.measured_ms = None

    def _run(self):
        for _ in range(self.reps):
            self.t.add_(1.0)

    def measure(self) -> float:
        """The gate's duration in ms, by events on the current (default) stream."""
        torch = self.torch
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        self._run()
        e1.record()
        e1.synchronize()
        return float(e0.elapsed_time(e1))

    def calibrate(self, target_ms: float) -> "Gate":
        """Set reps so that the gate lasts at least target_ms, and measure it."""
        self.reps = 16
        self.measure()  # warm
        self.ms_per_rep = self.measure() / self.reps
        self.reps = max(1, math.ceil(target_ms / self.ms_per_rep))
        self.measured_ms = self.measure()
        for _ in range(4):  # (never shorter than asked for: the clocks may have risen since the first measurement)
            if self.measured_ms >= target_ms:
                break
            self.reps = math.ceil(self.reps * 1.25 * target_ms / self.measured_ms)
            self.measured_ms = self.measure()
        assert self.measured_ms >= target_ms, (self.measured_ms, target_ms)
        return self

    def like(self) -> "Gate":
        """A second gate of the same length (another tensor: two streams never touch one)."""
        g = Gate(self.torch, self.reps)
        g.ms_per_rep, g.measured_ms = self.ms_per_rep, self.measured_ms
        return g

    def enqueue(self, stream):
        """The delay on `stream`, then an event recorded behind it: event.query() is False until the gate has run."""
        torch = self.torch
        with torch.cuda.stream(stream):
            self._run()
            ev = torch.cuda.Event()
            ev.record(stream)
        return ev


def device_bytes(torch, a):
    """A numpy array's bytes as a uint8 device tensor (on the current stream)."""
    import numpy as np
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def poisoned(torch, nbytes: int, pad: int):
    """An output buffer of nbytes + pad bytes of poison; torch's allocations are aligned to 16 B and more."""
    return torch.full((nbytes + pad,), POISON, dtype=torch.uint8, device="cuda")


class Run:
    """What run_on_side_stream (or on_default_stream) saw: result = what call() returned, host_s = the host time of
    call(), pending = the gate's event had not completed when call() returned, outputs = the used bytes of each
    output."""

    def __init__(self, result, host_s, pending, outputs):
        self.result, self.host_s, self.pending, self.outputs = result, host_s, pending, outputs


def on_default_stream(torch, call, inputs, outputs, fresh=None, before=None, after=None) -> Run:
    """Step 1 of the recipe: the same sequence on stream 0, waited for.  inputs: (buffer, staged) pairs of uint8 device
    tensors, the call reads buffer; outputs: (buffer, used bytes) pairs, buffer longer than used by its PAD."""
    if fresh:
        fresh()
    for buf, staged in inputs:
        buf.copy_(staged)
    for buf, _ in outputs:
        buf.fill_(POISON)
    if before:
        before(0)
    t0 = time.perf_counter()
    result = call(0)
    host_s = time.perf_counter() - t0
    if after:
        after(0)
    torch.cuda.synchronize()
    got = [buf.cpu().numpy() for buf, _ in outputs]
    for g, (_, used) in zip(got, outputs):
        assert (g[used:] == POISON).all(), "stream 0: bytes past the end were written"
    return Run(result, host_s, False, [g[:used].tobytes() for g, (_, used) in zip(got, outputs)])


def run_on_side_stream(torch, side, gate, call, inputs, outputs, expected=None, enqueue_only=True, fresh=None,
                       before=None, after=None) -> Run:
    """The recipe of the module docstring.  call(stream) makes the library call under test on the raw stream handle
    and returns what the wrapper returns.  fresh(): host-side preparation before anything is enqueued (a blocking
    rtx_accum_reset); before(stream) / after(stream): further library calls on the same stream behind the gate, before
    and after the call (the passes a reader reads, the resolve that makes a pass visible).  expected: the stream-0
    bytes of each output when the caller already has them (else step 1 runs here).

    Asserts (a) the outputs equal the stream-0 bytes and the PAD bytes kept their poison, and either (b)
    enqueue_only: the gate was still pending when call() returned (a gate that has finished by then proves nothing:
    the case fails), or (c) not enqueue_only: the gate had finished, that is the call synchronised its stream."""
    if expected is None:
        on_default_stream(torch, call, inputs, outputs, fresh, before, after)  # warms tables, layouts and the scratch
        expected = on_default_stream(torch, call, inputs, outputs, fresh, before, after).outputs
    default = torch.cuda.current_stream()
    assert default.cuda_stream == 0 and side.cuda_stream != 0
    if fresh:
        fresh()
    # 2. poison every input and output on stream 0; the side stream starts after it
    for buf, _ in list(inputs) + list(outputs):
        buf.fill_(POISON)
    side.wait_stream(default)
    # 3. the gate
    gate_event = gate.enqueue(side)
    with torch.cuda.stream(side):
        # 4. the real inputs, 5. the outputs poisoned again: both behind the gate
        for buf, staged in inputs:
            buf.copy_(staged, non_blocking=True)
        for buf, _ in outputs:
            buf.fill_(POISON)
        if before:
            before(side.cuda_stream)
        # 6. the call
        t0 = time.perf_counter()
        result = call(side.cuda_stream)
        host_s = time.perf_counter() - t0
        pending = not gate_event.query()
        if after:
            after(side.cuda_stream)
        # 7. the outputs as the stream sees them now
        clones = [buf.clone() for buf, _ in outputs]
    side.synchronize()  # this stream only
    got = [c.cpu().numpy() for c in clones]
    for i, (g, (_, used)) in enumerate(zip(got, outputs)):
        assert (g[used:] == POISON).all(), f"output {i}: bytes past the end were written"
        if g[:used].tobytes() != expected[i]:
            import numpy as np
            bad = np.nonzero(g[:used] != np.frombuffer(expected[i], np.uint8))[0]
            raise AssertionError(f"output {i}: {len(bad)} of {used} bytes differ from the stream-0 bytes, first at byte "
                                 f"{bad[0]}; {int((g[:used] == POISON).sum())} bytes are poison")
    if enqueue_only:
        assert pending, (f"vacuous: the gate ({gate.measured_ms:.2f} ms) had finished when the call returned after "
                         f"{host_s * 1e3:.3f} ms on the host: either the call waited for the device, or the gate is too short")
    else:
        assert not pending, "the call returned while the gate before it was still running: it did not synchronise its stream"
    return Run(result, host_s, pending, [g[:used].tobytes() for g, (_, used) in zip(got, outputs)])
