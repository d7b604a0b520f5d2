#!/usr/bin/env python
"""
profiles/accuracy/README.md from a run of tests/test_gpu_accuracy.py, tests/test_gpu_accuracy_loops.py,
tests/test_gpu_accuracy_consumers.py and tests/test_gpu_instances.py on the GPU: the modules write the figures they measured -- one pass per form (the
kernel's error against the extended-precision reference, the sequential fp64 pass's, their ratio, the loops' ln_new error),
every loop form over K = 2, 3, 10 and 40 iterations (the error of ln_new in units of K u max(1, max |ln|), beside the
comparison pass's), and every consumer of the posterior (error, the comparison pass's, the bound, undecided rows) -- as
tables; this wraps them with the text that explains the columns.
    python tools/accuracy_report.py [output.md [more pytest arguments]]
    python tools/accuracy_report.py --from-tables PREFIX [output.md]     the tables a run with MXM_ACCURACY_REPORT=PREFIX
                                                                         left (PREFIX, PREFIX.loops, PREFIX.consumers,
                                                                         PREFIX.instances)
    python tools/accuracy_report.py --instances PREFIX [output.md]       only the section "Every instance at its edges" of an
                                                                         existing report, from PREFIX.instances (a run of
                                                                         tests/test_gpu_instances.py alone)
    ... --note "TEXT"    (any form) a paragraph in front of that section's tables: what the run cost -- the wall time of the GPU
                         suite with and without the module, which no test measures
"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAD = """# Accuracy of the EM passes against an extended-precision reference

Written by `tools/accuracy_report.py` from `pytest -m gpu tests/test_gpu_accuracy.py tests/test_gpu_accuracy_loops.py
tests/test_gpu_accuracy_consumers.py` (MI355X).  One pass per form; `T` is
`colsum`, the M-step sums without their factor `p_h`; `u = 2^-53`; `rel(X) = max_h |X_h - T_exact,h| / T_exact,h` with
`T_exact` from `tests/_exact.py` (numpy.longdouble on the bits the kernel reads).  `T_seq` is a plain fp64 pass in
sequential order on the same inputs (for the log-space forms: `oracle.em_oracle.em_step`).  The tests assert
`rel(T_gpu) <= 8 * max(rel(T_seq), 4u)` and `rel(T_gpu) <= (R + H + 8) u`; `ln_new` and the posteriors are absolute errors,
asserted `<= 8 * max(the fp64 oracle's own error, u * max |value|)`.  The one-launch loops write no `colsum`: their rows
carry the `ln_new` error only.

"""
LOOPS = """
# The loops over K iterations

`tests/test_gpu_accuracy_loops.py`: every loop form run for K = 2, 3, 10 and 40 iterations (`tol = 0`) from the vectors
"dirichlet", "skewed" and "deep" (`ln p ~ U(-760, -690)`: subnormal or zero in linear space) on 96-row matrices, against
the long-double trajectory of `tests/_exact_traj.py`.  Each cell is `max_h |ln_new - ln_exact,K|` of the loop and of the
comparison pass (the same recurrence in plain fp64), both in units of the floor `K u max(1, max_h |ln_exact,K|)`; the test asserts
`error <= 8 * max(comparison pass, floor)`.

"""
CONSUMERS = """
# The consumers of the posterior

`tests/test_gpu_accuracy_consumers.py`: the votes, the logaddexp fold, the read assignment, the posterior under the "deep"
vector and the two small vector entries against `tests/_exact_consumers.py` (numpy.longdouble on the bits the kernels read).
`error` is the largest absolute error over the entries whose exact value is finite, `comparison pass` the same figure of the
plain fp64 numpy restatement (`numpy.logaddexp` chains, `oracle.em_oracle.logsumexp`), `bound` =
`8 * max(comparison pass, u * max |value|)`; the test asserts `error <= bound` and the reference's pattern of `-inf` / NaN.
The rows of the decisions (`best`, `assigned`) carry `d` = twice the bound of the values they are taken on in the `bound`
column and the number of undecided rows (a second answer within `d`: at most 1 % per case); every other row must carry the
exact answer.  "orphans below t" are rows supported only by columns with `ln p < t`: their linear row sum
`sum_h p_h P_rh` is a small normal number made of gradually underflowing products (-700), subnormal (-715, -738) or zero
(-750); the kernels redo every row whose sum is below `2^-960` in log space.  Those rows' lines give the error alone (the
assertion is the line of the whole matrix).

"""
INSTANCES = """
# Every instance at its edges

`tests/test_gpu_instances.py`: every kernel instance the width dispatchers of `mixemt_hip.hip` compile
(`tests/_instances.py` restates each site's formula from the width to the instance), run at the first and at the last width
that reach it -- one call per case on 3, 37 or 64 rows, under the rule of the entry's own tests: `colsum` under the two
bounds above; `exp` in ulp for `mxm_linearize`; absolute errors of posterior and `ln_new` for `mxm_em_step` and the
one-launch loops (three iterations); exact labels and votes for the argmax entries; the encoder's round trip and the
builders bit for bit ("other" then says what the case measured).

"""


NOTE = [""]


def write_report(out, parts):
    with open(out, "w") as dst:
        for head, part in zip((HEAD, LOOPS, CONSUMERS, INSTANCES), parts):
            if head is INSTANCES and not os.path.exists(part):       # (a run without tests/test_gpu_instances.py)
                continue
            dst.write(head + (NOTE[0] if head is INSTANCES else ""))
            with open(part) as src:
                dst.write(src.read())


def replace_instances(out, table):
    """The section "Every instance at its edges" of an existing report: replaced, or appended."""
    with open(out) as src:
        text = src.read()
    at = text.find(INSTANCES.lstrip("\n").split("\n")[0])
    if at >= 0:
        text = text[:at].rstrip("\n") + "\n"
    with open(table) as src:
        text += INSTANCES + NOTE[0] + src.read()
    with open(out, "w") as dst:
        dst.write(text)


def main():
    if "--note" in sys.argv:
        at = sys.argv.index("--note")
        NOTE[0] = sys.argv[at + 1].strip() + "\n\n"
        del sys.argv[at:at + 2]
    if len(sys.argv) > 2 and sys.argv[1] == "--from-tables":
        out = os.path.abspath(sys.argv[3]) if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "accuracy", "README.md")
        write_report(out, [sys.argv[2], sys.argv[2] + ".loops", sys.argv[2] + ".consumers", sys.argv[2] + ".instances"])
        return 0
    if len(sys.argv) > 2 and sys.argv[1] == "--instances":
        out = os.path.abspath(sys.argv[3]) if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "accuracy", "README.md")
        replace_instances(out, sys.argv[2] + ".instances")
        return 0
    out = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "accuracy", "README.md")
    table = out + ".table"
    env = dict(os.environ, MXM_ACCURACY_REPORT=table)
    rc = subprocess.call([sys.executable, "-m", "pytest", "-m", "gpu", "-q", os.path.join(ROOT, "tests", "test_gpu_accuracy.py"),
                          os.path.join(ROOT, "tests", "test_gpu_accuracy_loops.py"),
                          os.path.join(ROOT, "tests", "test_gpu_accuracy_consumers.py"),
                          os.path.join(ROOT, "tests", "test_gpu_instances.py")] + sys.argv[2:], cwd=ROOT, env=env)
    parts = [table, table + ".loops", table + ".consumers", table + ".instances"]
    if all(os.path.exists(p) for p in parts) and rc == 0:          # (a failed or interrupted run leaves the committed tables alone)
        write_report(out, parts)
    for part in parts:
        if os.path.exists(part):
            os.remove(part)
    return rc


if __name__ == "__main__":
    sys.exit(main())
