"""
The stream contract of the C ABI (include/mixemt_hip.h: "`stream` is a hipStream_t ...; every call only enqueues work on
it unless stated otherwise"), checked on a side stream that is still BUSY when the library is called.  Not a conftest: a
helper that tests/test_gpu_stream_contract.py and tools/stream_contract_report.py share.

A case (tests/_stream_cases.py) is one call of one entry through one host route.  It is run three ways on a
torch.cuda.Stream() -- torch creates its streams non-blocking, so the legacy default stream does not order itself against
them, and a launch that went to nullptr instead of the caller's stream runs at once, on the decoys:

  quiet   inputs in place, synchronise, the call on the side stream, synchronise: the reference (same code path, same
          launch shape as the busy run, hence compared bit for bit where the quiet run reproduces itself);
  busy    every input with a payload holds its decoy, every other buffer its real start value (address-bearing inputs are
          identical in decoy and real input; outputs hold their sentinel, counters that the call uses as an offset a small
          in-range value; workspaces are zeroed); on the side stream a delay kernel, the `gate` event, then device-to-device
          copies that put the real inputs and the outputs' start values in place (again: what ran ahead of its place is
          overwritten); the call;
          straight after it returns -- before any synchronise -- device-to-device snapshots of every output are enqueued on
          the side stream and every host input array is overwritten with the decoy's tables;
  graph   the call captured on the side stream (one stream, a linear chain), the buffers put back, one replay.

A decoy differs from the real input only in values that no address is computed from (floating-point payloads are NaN,
integer payloads are another valid problem's), and a buffer without a decoy holds its real value from the start: offsets,
pointer arrays, codes, CIGARs, row lists and sizes are never anything but themselves, so work that runs ahead of its place
in the stream computes a wrong result from in-range addresses.  Case() asserts that every buffer is an output, an input
with a decoy, or an input left identical (named in `identical`).
"""
import time

import numpy

DELAY_ENQUEUE_MS = 200.0                     # entries that must only enqueue: a condition, not a measurement
DELAY_WAITING_MS = 50.0                      # entries whose header says that they wait

_cycles_per_ms = None


def sentinel(shape, dtype):
    """An output nobody has written: every byte 0xFF (a double reads as NaN, an integer as -1)."""
    out = numpy.empty(shape, dtype=dtype)
    out.view(numpy.uint8).reshape(-1)[:] = 0xFF
    return out


def nan_like(values):
    return numpy.full_like(numpy.asarray(values), numpy.nan)


class Case:
    """
    entry, route   the C ABI entry and the host route through it that the case takes
    klass          "A" only enqueues, capturable; "B" only enqueues, uploads host arrays or takes stream-ordered memory;
                   "C" waits (its header says so)
    bufs           {name: numpy array}: every device buffer's value when the call starts (an output: its sentinel)
    decoy          {name: numpy array}: the decoys of the inputs that carry a payload
    identical      the names of the inputs that are identical in decoy and real input (offsets, codes, row lists, sizes)
    outs           the names of the buffers the call writes
    scratch        {name: bytes}: workspaces (contents unspecified, never compared)
    host           {name: (real, decoy)} host input arrays, or a function of the device pointers that returns the pair (an
                   array OF device pointers); host_outs {name: zeroed array} host outputs (state_host)
    call(p, h, stream) -> return code; p: {name: device pointer}, h: {name: numpy array on the host}
    setup(lib)     tuning setters the route needs (undone with mxm_reset_tuning after every call)
    """

    def __init__(self, entry, route, klass, call, bufs, decoy, outs, scratch=None, host=None, host_outs=None, setup=None,
                 identical=None):
        assert klass in ("A", "B", "C"), klass
        self.entry, self.route, self.klass, self.call = entry, route, klass, call
        self.bufs = {k: numpy.ascontiguousarray(v) for k, v in bufs.items()}
        self.decoy = {k: numpy.ascontiguousarray(v) for k, v in decoy.items()}
        self.outs = list(outs)
        self.scratch = dict(scratch or {})
        self.host = dict(host or {})
        self.host_outs = dict(host_outs or {})
        self.setup = setup
        # every buffer is an output, an input with a decoy, or an input left identical: nothing else exists
        self.identical = sorted(set(self.bufs) - set(self.decoy) - set(self.outs)) if identical is None else sorted(identical)
        assert set(self.identical) | set(self.decoy) | set(self.outs) == set(self.bufs), (entry, route)
        assert not (set(self.identical) & (set(self.decoy) | set(self.outs))), (entry, route, self.identical)
        self.canon = lambda out: out                   # what of the outputs is compared (a producer's free placement decoded)
        for name, dec in self.decoy.items():
            real = self.bufs[name]
            assert dec.dtype == real.dtype and dec.shape == real.shape, (entry, route, name)
        assert set(self.outs) <= set(self.bufs), (entry, route)

    @property
    def id(self):
        return "%s[%s]" % (self.entry, self.route)

    @property
    def delay_ms(self):
        return DELAY_WAITING_MS if self.klass == "C" else DELAY_ENQUEUE_MS


def load_lib():
    from mixemt_amd import _lib
    return _lib.load()


def cycles_per_ms():
    """The delay kernel's rate, measured once per session with events around the kernel itself."""
    global _cycles_per_ms
    if _cycles_per_ms is None:
        import torch
        side = torch.cuda.Stream()
        probe = 20000000
        with torch.cuda.stream(side):
            torch.cuda._sleep(1000000)                       # (its code object loads here, not inside the timing)
            side.synchronize()
            best = None
            for _ in range(3):
                start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record(side)
                torch.cuda._sleep(probe)
                stop.record(side)
                side.synchronize()
                ms = start.elapsed_time(stop)
                best = ms if best is None else min(best, ms)
        assert best > 0.5, "the delay kernel returned at once (%.3f ms for %d cycles)" % (best, probe)
        _cycles_per_ms = probe / best
    return _cycles_per_ms


def _dev(values):
    import torch
    return torch.from_numpy(numpy.ascontiguousarray(values).view(numpy.uint8).reshape(-1).copy()).cuda()


class Staged:
    """A case's staging tensors on the device (bytes): the real start values and the decoys.  Made once per case."""

    def __init__(self, case):
        self.case = case
        self.real = {k: _dev(v) for k, v in case.bufs.items()}
        self.decoy = {k: _dev(v) for k, v in case.decoy.items()}


class Run:
    """One set of working buffers for a case: device buffers, workspaces, snapshots, host arrays."""

    def __init__(self, staged, pinned=False):
        import torch
        self.staged, self.case = staged, staged.case
        case = self.case
        self.work = {k: torch.empty_like(v) for k, v in staged.real.items()}
        self.snap = {k: torch.empty_like(staged.real[k]) for k in case.outs}
        self.scratch = {k: torch.empty(max(int(n), 16), dtype=torch.uint8, device="cuda") for k, n in case.scratch.items()}
        self.host, self._pins = {}, []
        for name in case.host:
            real, _ = self.host_pair(name)
            if pinned:
                pin = torch.empty(max(real.nbytes, 1), dtype=torch.uint8, pin_memory=True)
                assert pin.is_pinned()
                self._pins.append(pin)
                arr = pin.numpy()[:real.nbytes].view(real.dtype).reshape(real.shape)
            else:
                arr = numpy.empty_like(real)
            arr[...] = real
            self.host[name] = arr
        for name, template in case.host_outs.items():
            self.host[name] = numpy.zeros_like(template)
        self.host_ms, self.gate_pending, self.rc = None, None, None

    def host_pair(self, name):
        spec = self.case.host[name]
        real, dec = spec(self.pointers()) if callable(spec) else spec
        real, dec = numpy.ascontiguousarray(real), numpy.ascontiguousarray(dec)
        assert dec.dtype == real.dtype and dec.shape == real.shape, (self.case.id, name)
        return real, dec

    def pointers(self):
        p = {k: v.data_ptr() for k, v in self.work.items()}
        p.update({k: v.data_ptr() for k, v in self.scratch.items()})
        return p

    def place(self, decoys):
        """On the current stream: every buffer's start value, with the decoys in the inputs' place if asked."""
        for name, buf in self.work.items():
            src = self.staged.decoy.get(name) if decoys else None
            buf.copy_(self.staged.real[name] if src is None else src, non_blocking=True)
        for buf in self.scratch.values():
            buf.zero_()

    def set_host(self, decoys):
        for name in self.case.host:
            real, dec = self.host_pair(name)
            self.host[name][...] = dec if decoys else real

    def invoke(self, lib, stream):
        if self.case.setup is not None:
            self.case.setup(lib)
        try:
            begin = time.perf_counter()
            rc = self.case.call(self.pointers(), self.host, stream.cuda_stream)
            self.host_ms = (time.perf_counter() - begin) * 1e3
        finally:
            lib.mxm_reset_tuning()
        self.rc = rc
        assert rc == 0, (self.case.id, rc, lib.mxm_last_error())

    def outputs(self, which=None):
        """{name: bytes on the host} of the outputs (or of the snapshots), plus the host outputs."""
        src = self.work if which is None else which
        out = {k: src[k].cpu().numpy().copy() for k in self.case.outs}
        if which is None:
            for name in self.case.host_outs:
                out["host:" + name] = self.host[name].view(numpy.uint8).reshape(-1).copy()
        return out


def quiet_run(lib, staged, decoys=False):
    import torch
    run = Run(staged)
    side = torch.cuda.Stream()
    run.place(decoys)
    run.set_host(decoys)
    torch.cuda.synchronize()
    run.invoke(lib, side)
    side.synchronize()
    torch.cuda.synchronize()
    return run.outputs()


class BusyRun:
    """The busy run in its steps, so that two of them can be interleaved on two streams from one host thread."""

    def __init__(self, lib, staged, pinned=False):
        import torch
        self.lib, self.run = lib, Run(staged, pinned)
        self.side = torch.cuda.Stream()
        self.gate = torch.cuda.Event()
        self.delay_ms = staged.case.delay_ms

    def stage(self):
        self.run.place(True)                           # step 1: the decoys; every other buffer is itself from the start
        self.run.set_host(False)

    def enqueue_delay(self):
        import torch
        with torch.cuda.stream(self.side):
            torch.cuda._sleep(int(self.delay_ms * cycles_per_ms()))
            self.gate.record(self.side)
            for name, buf in self.run.work.items():
                buf.copy_(self.run.staged.real[name], non_blocking=True)

    def call(self):
        import torch
        run = self.run
        run.invoke(self.lib, self.side)
        run.gate_pending = not self.gate.query()
        with torch.cuda.stream(self.side):
            for name in run.case.outs:
                run.snap[name].copy_(run.work[name], non_blocking=True)
        run.set_host(True)

    def finish(self):
        import torch
        self.side.synchronize()
        torch.cuda.synchronize()
        return self.run.outputs(), self.run.outputs(self.run.snap)


def busy_run(lib, staged, pinned=False):
    """-> (outputs, snapshots, host milliseconds of the call, gate still pending at return)."""
    import torch
    busy = BusyRun(lib, staged, pinned)
    busy.stage()
    torch.cuda.synchronize()
    busy.enqueue_delay()
    busy.call()
    outs, snaps = busy.finish()
    return outs, snaps, busy.run.host_ms, busy.run.gate_pending


def graph_run(lib, staged):
    """The call captured on one stream, the buffers put back, one replay -> outputs."""
    import torch
    run = Run(staged)
    side = torch.cuda.Stream()
    run.place(False)
    run.set_host(False)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side, capture_error_mode="thread_local"):
        run.invoke(lib, torch.cuda.current_stream())
    run.place(True)
    run.place(False)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    return run.outputs()


def same(case, got, want):
    """None if the two output sets agree bit for bit, else the first output that does not."""
    for name in want:
        if not numpy.array_equal(got[name], want[name]):
            return name
    return None
