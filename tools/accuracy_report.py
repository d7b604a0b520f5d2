#!/usr/bin/env python
"""
profiles/accuracy/README.md from a run of tests/test_gpu_accuracy.py on the GPU: the module writes the figures it measured
(per form, width, rows and proportion vector: the kernel's error against the extended-precision reference, the sequential
fp64 pass's, their ratio, the loops' ln_new error) as a table; this wraps it with the text that explains the columns.
    python tools/accuracy_report.py [output.md [more pytest arguments]]
"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAD = """# Accuracy of the EM passes against an extended-precision reference

Written by `tools/accuracy_report.py` from `pytest -m gpu tests/test_gpu_accuracy.py` (MI355X).  One pass per form; `T` is
`colsum`, the M-step sums without their factor `p_h`; `u = 2^-53`; `rel(X) = max_h |X_h - T_exact,h| / T_exact,h` with
`T_exact` from `tests/_exact.py` (numpy.longdouble on the bits the kernel reads).  `T_seq` is a plain fp64 pass in
sequential order on the same inputs (for the log-space forms: `oracle.em_oracle.em_step`).  The tests assert
`rel(T_gpu) <= 8 * max(rel(T_seq), 4u)` and `rel(T_gpu) <= (R + H + 8) u`; `ln_new` and the posteriors are absolute errors,
asserted `<= 8 * max(the fp64 oracle's own error, u * max |value|)`.  The one-launch loops write no `colsum`: their rows
carry the `ln_new` error only.

"""


def main():
    out = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "accuracy", "README.md")
    table = out + ".table"
    env = dict(os.environ, MXM_ACCURACY_REPORT=table)
    rc = subprocess.call([sys.executable, "-m", "pytest", "-m", "gpu", "-q", os.path.join(ROOT, "tests", "test_gpu_accuracy.py")] + sys.argv[2:],
                         cwd=ROOT, env=env)
    if os.path.exists(table):
        if rc == 0:                                    # (a failed or interrupted run leaves the committed table alone)
            with open(table) as src, open(out, "w") as dst:
                dst.write(HEAD + src.read())
        os.remove(table)
    return rc


if __name__ == "__main__":
    sys.exit(main())
