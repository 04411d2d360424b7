"""Late inputs on a side stream: a harness that makes a stream-ordering violation deterministic (a
helper module for tests/test_gpu_streams.py, not a conftest; torch only, no hj3d).

include/hj3d.h promises that every call is enqueued on the context's stream. On torch's default
stream that cannot be checked: everything is ordered there anyway. Here every input of the call under
test first holds a *decoy*; inside `with torch.cuda.stream(s)` the harness then enqueues, back to
back and without a host synchronisation,

    a delay  ->  input.copy_(real data)  ->  the call(s) under test  ->  clones of the outputs
             ->  input.copy_(decoy)                       (the clobber)

Work the call puts on any other stream starts at once, since the other streams are idle while `s`
still runs the delay: it reads the decoy. Work that runs late on another stream reads the decoy again,
or is missed by the clone. Either way the result, read through the library's own synchronous getters
with no explicit synchronisation, differs from the CPU reference of the real data.

For a call that is fully asynchronous the harness also asserts that the delay is still running when
the enqueue sequence has returned (`not end_event.query()`); otherwise the case has proved nothing and
fails as DelayTooShort ("delay too short"), which is also what a host synchronisation that slipped
into the call produces. A call with a documented host wait inside cannot meet that condition: its late
input proves that the wait is on `s` (a wait on another stream returns at once, and what follows reads
the decoy), its tail is covered by the clone and the clobber only as far as the host runs ahead.

The delay is ordinary torch work on `s` (sorts of a scratch tensor), calibrated with torch events on
`s` by doubling the repeat count until it measures at least the target, max(MIN_DELAY_MS,
HOST_FACTOR x the host wall time of the case's enqueue sequence in its warm-up). 5 ms is some hundred
times the tens of microseconds between an enqueue and its start on an idle stream; the factor 4 lets
the host be slower in the counted call than in the warm-up.

Before the counted call a case runs the same sequence as a warm-up (twice: the first grows the
library's scratch, which synchronises the device; the second is timed) and synchronises, then runs
its `reset` (the call once on the decoy, or a table cleared) so that neither the result slot nor an
output buffer still holds the real result, and fills the outputs with a canary."""
import time

MIN_DELAY_MS = 5.0
HOST_FACTOR = 4.0
CANARY = 0x5A5A5A5A
SCRATCH = 1 << 23  # int32 elements a delay step sorts: ~1 ms of device work against ~0.05 ms to enqueue


class DelayTooShort(AssertionError):
    """The delay had ended when the enqueue sequence returned: nothing was proved (or the call waited)."""


def target_ms(host_ms: float) -> float:
    return max(MIN_DELAY_MS, HOST_FACTOR * host_ms)


def too_short(name, delay_ms, host_ms) -> DelayTooShort:
    return DelayTooShort(f"delay too short: {name}: the {delay_ms:.1f} ms delay had ended when the enqueue sequence "
                         f"returned after {host_ms:.2f} ms on the host (a host wait inside an asynchronous call?)")


class Late:
    """One late input: `tensor` (what the call reads), the real data and the decoy beside it."""

    def __init__(self, tensor, real, decoy):
        assert tensor.shape == real.shape == decoy.shape and tensor.dtype == real.dtype == decoy.dtype
        self.tensor, self.real, self.decoy = tensor, real, decoy

    @classmethod
    def of(cls, real_np, decoy_np):
        """A fresh input from two host arrays of one shape (uint32 or 64-bit words)."""
        import torch
        real, decoy = to_device(real_np), to_device(decoy_np)
        late = cls(decoy.clone(), real, decoy)
        torch.cuda.synchronize()  # (the clone ran on the caller's current stream: done before any stream uses it)
        return late

    @classmethod
    def wrap(cls, tensor, real_np, decoy_np):
        """An input the test world already holds (tensor keeps its address: relations point at it)."""
        import torch
        late = cls(tensor, to_device(real_np), to_device(decoy_np))
        torch.cuda.synchronize()
        return late


def to_device(a):
    import numpy as np
    import torch
    a = np.ascontiguousarray(a)
    view = {4: np.int32, 8: np.int64}[a.dtype.itemsize]
    return torch.from_numpy(a.view(view)).cuda()


class Delay:
    """Torch work on `stream` of a calibrated length."""

    def __init__(self, stream):
        import torch
        self.stream = stream
        with torch.cuda.stream(stream):
            self.scratch = torch.randint(0, 1 << 30, (SCRATCH,), dtype=torch.int32, device="cuda")
        stream.synchronize()
        self.measured = {}  # repeat count -> ms by torch events on the stream
        self._measure(1)    # (the sort's own temporaries enter the caching allocator)

    def _work(self, reps):
        import torch
        for _ in range(reps):
            torch.sort(self.scratch)

    def _measure(self, reps):
        import torch
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(self.stream):
            a.record()
            self._work(reps)
            b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def reps_for(self, ms):
        reps = 1
        while True:
            if reps not in self.measured:
                self.measured[reps] = self._measure(reps)
            if self.measured[reps] >= ms:
                return reps
            assert reps < 1 << 16, "the delay does not grow with its repeat count"
            reps *= 2

    def enqueue(self, ms):
        """Called with `stream` current: the delay, and the event that ends it. Returns (event, measured ms)."""
        import torch
        reps = self.reps_for(ms)
        self._work(reps)
        end = torch.cuda.Event()
        end.record(self.stream)
        return end, self.measured[reps]


class Outcome:
    def __init__(self, clones, delay_ms, warm_host_ms, host_ms, still_running):
        self.clones, self.delay_ms, self.warm_host_ms, self.host_ms = clones, delay_ms, warm_host_ms, host_ms
        self.still_running = still_running


class Harness:
    def __init__(self, stream):
        self.stream = stream
        self.delay = Delay(stream)
        self.log = {}  # case name -> (measured delay ms, warm-up host ms, counted host ms, delay still running)

    def host(self, t):
        """A host copy of a device tensor, ordered on the harness stream (call it after the library's
        synchronous getter, so that the getter is the only thing the check relies on)."""
        import torch
        with torch.cuda.stream(self.stream):
            return t.cpu().numpy()

    def _sequence(self, inputs, call, outputs, before_clobber, end):
        t0 = time.perf_counter()
        for i in inputs:
            i.tensor.copy_(i.real, non_blocking=True)
        call()
        clones = [o.clone() for o in outputs]
        still = None
        if before_clobber is not None:  # (a documented host wait: the condition is sampled before it)
            still = end is None or not end.query()
            host_ms = (time.perf_counter() - t0) * 1e3
            before_clobber()
        for i in inputs:
            i.tensor.copy_(i.decoy, non_blocking=True)
        if before_clobber is None:
            host_ms = (time.perf_counter() - t0) * 1e3
            still = end is None or not end.query()
        return clones, host_ms, still

    def run(self, name, inputs, call, outputs=(), fully_async=True, before_clobber=None, reset=None):
        """The late-input sequence for one case. call(): the hj3d call(s) under test, nothing fetched.
        outputs: the device tensors the call writes. before_clobber(): what must come between the call and
        the clobber (Table.finish of a nested build). reset(): run synchronously after the warm-up, on the
        decoy. Returns an Outcome; raises DelayTooShort for a fully asynchronous case whose delay had ended."""
        import torch
        s = self.stream
        with torch.cuda.stream(s):
            for _ in range(2):
                _, warm_ms, _ = self._sequence(inputs, call, outputs, before_clobber, None)
                torch.cuda.synchronize()
            for i in inputs:
                i.tensor.copy_(i.decoy)
            torch.cuda.synchronize()
            if reset is not None:
                reset()
            for o in outputs:
                o.fill_(CANARY)
            torch.cuda.synchronize()
            end, delay_ms = self.delay.enqueue(target_ms(warm_ms))
            clones, host_ms, still = self._sequence(inputs, call, outputs, before_clobber, end)
        self.log[name] = (delay_ms, warm_ms, host_ms, still)
        print(f"stream-order {name}: delay {delay_ms:.1f} ms, host enqueue {warm_ms:.3f} ms (warm-up) "
              f"{host_ms:.3f} ms (counted), delay still running: {still}, fully asynchronous: {fully_async}")
        if fully_async and not still:
            raise too_short(name, delay_ms, host_ms)
        return Outcome(clones, delay_ms, warm_ms, host_ms, still)
