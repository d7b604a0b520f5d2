#!/usr/bin/env python
"""
profiles/accuracy/README.md from a run of tests/test_gpu_accuracy.py, tests/test_gpu_accuracy_loops.py and
tests/test_gpu_accuracy_consumers.py on the GPU: the modules write the figures they measured -- one pass per form (the
kernel's error against the extended-precision reference, the sequential fp64 pass's, their ratio, the loops' ln_new error),
every loop form over K = 2, 3, 10 and 40 iterations (the error of ln_new in units of K u max(1, max |ln|), beside the
comparison pass's), and every consumer of the posterior (error, the comparison pass's, the bound, undecided rows) -- as
tables; this wraps them with the text that explains the columns.
    python tools/accuracy_report.py [output.md [more pytest arguments]]
    python tools/accuracy_report.py --from-tables PREFIX [output.md]     the tables a run with MXM_ACCURACY_REPORT=PREFIX
                                                                         left (PREFIX, PREFIX.loops, PREFIX.consumers)
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


def write_report(out, parts):
    with open(out, "w") as dst:
        for head, part in zip((HEAD, LOOPS, CONSUMERS), parts):
            with open(part) as src:
                dst.write(head + src.read())


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--from-tables":
        out = os.path.abspath(sys.argv[3]) if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "accuracy", "README.md")
        write_report(out, [sys.argv[2], sys.argv[2] + ".loops", sys.argv[2] + ".consumers"])
        return 0
    out = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "accuracy", "README.md")
    table = out + ".table"
    env = dict(os.environ, MXM_ACCURACY_REPORT=table)
    rc = subprocess.call([sys.executable, "-m", "pytest", "-m", "gpu", "-q", os.path.join(ROOT, "tests", "test_gpu_accuracy.py"),
                          os.path.join(ROOT, "tests", "test_gpu_accuracy_loops.py"),
                          os.path.join(ROOT, "tests", "test_gpu_accuracy_consumers.py")] + sys.argv[2:], cwd=ROOT, env=env)
    parts = [table, table + ".loops", table + ".consumers"]
    if all(os.path.exists(p) for p in parts) and rc == 0:          # (a failed or interrupted run leaves the committed tables alone)
        write_report(out, parts)
    for part in parts:
        if os.path.exists(part):
            os.remove(part)
    return rc


if __name__ == "__main__":
    sys.exit(main())
