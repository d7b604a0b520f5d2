#!/usr/bin/env python
"""
profiles/streams/README.md: what every case of tests/_stream_cases.py did on a busy side stream (tests/_busy_stream.py) --
its class, the host time of the busy call, whether the gate behind the delay was still pending when the call returned, the
outcome with the host arrays in pageable and in pinned memory, the graph run's outcome for class A, and whether the
comparison with the quiet run was bit for bit.  Nothing is asserted here: tests/test_gpu_stream_contract.py asserts; this
records the figures (the host times are what nobody had measured).  A mismatch is written down as such; any other error
ends the run at once, with nothing further started on the device.
    python tools/stream_contract_report.py [output.md [entry ...]]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HEAD = """# The stream contract of the C ABI on a busy side stream

Written by `tools/stream_contract_report.py` (MI355X).  One line per case of `tests/_stream_cases.py`: one call of one entry
through one host route on a non-blocking side stream, behind a delay kernel of %(a).0f ms (classes A and B: entries that
only enqueue) or %(c).0f ms (class C: entries whose header says that they wait) and device-to-device copies that put the
real inputs in place; until then every input with a payload holds a decoy (offsets, codes and row lists are themselves).  Delay kernel: %(rate).0f cycles per ms, measured with events
around the kernel itself.

* `host ms`: wall time of the call on the host (pageable host arrays).  An entry that only enqueues returns in microseconds
  to about a millisecond; the tests ask for less than half the delay.
* `gate`: whether the event recorded behind the delay was still pending when the call returned.
* `pageable` / `pinned`: the busy run against the quiet run, the host arrays overwritten with another problem's tables as
  soon as the call returns (`-`: the entry takes no host array).
* `graph`: the call captured on one stream and replayed once (class A only).
* `bitwise`: the quiet run reproduces itself bit for bit (`decoded`: after decoding the records a bump allocator placed).

| case | class | host ms | gate | pageable | pinned ms | pinned | graph | bitwise |
|---|---|---|---|---|---|---|---|---|
"""


def main():
    import numpy
    import torch
    import _busy_stream as bs
    import _stream_cases as sc
    out = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "streams", "README.md")
    only = set(sys.argv[2:])
    lib = bs.load_lib()
    rate = bs.cycles_per_ms()
    lines = []
    for entry, route, klass, build in sc.TABLE:
        if only and entry not in only:
            continue
        case = build(lib)
        staged = bs.Staged(case)
        want = bs.quiet_run(lib, staged)
        again = bs.quiet_run(lib, staged)
        raw = all(numpy.array_equal(again[k], want[k]) for k in want)
        bitwise = "yes" if raw else ("decoded" if bs.same(case, case.canon(again), case.canon(want)) is None else "NO")

        def verdict(outs, snaps=None):
            bad = bs.same(case, case.canon(outs), case.canon(want))
            if bad is None and snaps is not None:
                bad = next((k for k in case.outs if not numpy.array_equal(snaps[k], outs[k])), None)
                bad = None if bad is None else "snapshot of " + bad
            return "ok" if bad is None else "MISMATCH (%s)" % bad
        outs, snaps, host_ms, pending = bs.busy_run(lib, staged, pinned=False)
        cells = [case.id, klass, "%.3f" % host_ms, "pending" if pending else "passed", verdict(outs, snaps)]
        if case.host:
            outs, snaps, pin_ms, _ = bs.busy_run(lib, staged, pinned=True)
            cells += ["%.3f" % pin_ms, verdict(outs, snaps)]
        else:
            cells += ["-", "-"]
        if klass == "A":
            try:
                cells.append(verdict(bs.graph_run(lib, staged)))
            except RuntimeError as err:                # a capture the runtime refuses is a finding; anything else ends the run
                if "capture" not in str(err).lower():
                    raise
                cells.append("REFUSED (%s)" % str(err).splitlines()[0][:80])
        else:
            cells.append("-")
        cells.append(bitwise)
        line = "| " + " | ".join(cells) + " |"
        print(line, flush=True)
        lines.append(line)
        del staged
        torch.cuda.empty_cache()
    sc.close_exchange()
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as dst:
        dst.write(HEAD % {"a": bs.DELAY_ENQUEUE_MS, "c": bs.DELAY_WAITING_MS, "rate": rate} + "\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
