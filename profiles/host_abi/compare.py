"""
Parent against branch from the raw outputs in this directory (small_runs_{parent,branch}_N.txt of
tools/time_small_runs.py, bench_{parent,branch}_N.json of bench.py): per line the median of each side, the parent's own
run-to-run spread, and whether the branch is within the larger of that spread and 2 % of the parent.

    python profiles/host_abi/compare.py > profiles/host_abi/comparison.md
"""
import glob
import json
import os
import re
import statistics

HERE = os.path.dirname(os.path.abspath(__file__))
LINE = re.compile(r"^\s*(\d+) rows \(\s*[\d.]+ MB\)\s+(.+?)\s+(\d+) restart-iterations\s+([\d.]+) ms\s+([\d.]+) us per")


def small_runs(tag):
    """(rows, route) -> us per restart-iteration of every warm run (a route's first run in a process is dropped where
    the tool times it twice: it carries the code object's load)."""
    out = {}
    for path in sorted(glob.glob(os.path.join(HERE, "small_runs_%s_*.txt" % tag))):
        seen = {}
        for line in open(path):
            m = LINE.match(line)
            if m:
                seen.setdefault((int(m.group(1)), m.group(2)), []).append(float(m.group(5)))
        for key, vals in seen.items():
            out.setdefault(key, []).extend(vals[1:] if len(vals) > 1 else vals)
    return out


def bench(tag):
    vals = {}
    for path in sorted(glob.glob(os.path.join(HERE, "bench_%s_*.json" % tag))):
        lines = [ln for ln in open(path) if ln.lstrip().startswith("{")]
        rec = json.loads(lines[-1])
        for key in ("ms_per_step", "value"):
            if isinstance(rec.get(key), (int, float)):
                vals.setdefault(key, []).append(float(rec[key]))
    return vals


def row(name, parent, branch, higher_is_better=False):
    p, b = statistics.median(parent), statistics.median(branch)
    spread = (max(parent) - min(parent)) / p
    margin = max(spread, 0.02)
    ok = b >= p * (1 - margin) if higher_is_better else b <= p * (1 + margin)
    return "| %s | %.4g | %.4g | %+.1f %% | %.1f %% | %s |" % (name, p, b, 100 * (b / p - 1), 100 * spread, "yes" if ok else "NO")


def main():
    print("| measurement | parent (median) | branch (median) | branch - parent | parent's spread | within max(spread, 2 %) |")
    print("|---|---|---|---|---|---|")
    sp, sb = small_runs("parent"), small_runs("branch")
    for key in sorted(sp):
        if key in sb:
            print(row("%d rows, %s, us per restart-iteration" % key, sp[key], sb[key]))
    bp, bb = bench("parent"), bench("branch")
    for key in sorted(bp):
        if key in bb:
            print(row("bench.py `%s`" % key, bp[key], bb[key], higher_is_better=(key == "value")))


if __name__ == "__main__":
    main()
