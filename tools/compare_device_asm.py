"""
Compare the device code of two builds of csrc/mixemt_hip.hip symbol by symbol.

    hipcc <the library's flags without -shared> --cuda-device-only -S mixemt_amd/csrc/mixemt_hip.hip -o a.s    (each tree)
    python tools/compare_device_asm.py a.s b.s

A function's text is everything from its label to its end marker, which includes its kernel descriptor (the
.amdhsa_kernel block: registers, LDS, scratch).
Local labels carry the function's ordinal in the file, which moves when the order of instantiation does, so the
ordinals are dropped before comparing.  Prints the counts and every symbol that differs; exit status 1 if any does.
"""
import re
import sys


def functions(path):
    funcs, kernels = {}, set()
    name, body = None, None
    for line in open(path):
        m = re.match(r"^\s*\.amdhsa_kernel\s+(\S+)", line)
        if m:
            kernels.add(m.group(1))
        m = re.match(r"^([A-Za-z_$][\w$.]*):\s*(;.*)?$", line)
        if name is None and m and not m.group(1).startswith(".L"):
            name, body = m.group(1), []
        elif name is not None and re.match(r"^\.Lfunc_end\d+:", line):
            text = re.sub(r"\.L(BB|tmp|func_begin|func_end|JTI)\d+", r".L\1", "".join(body))
            funcs[name] = re.sub(r"[ \t]+", " ", text)
            name = None
        elif name is not None:
            body.append(line)
    return funcs, kernels


def main(a_path, b_path):
    a, ka = functions(a_path)
    b, kb = functions(b_path)
    print("functions: %d / %d, kernels: %d / %d" % (len(a), len(b), len(ka), len(kb)))
    bad = 0
    for sym in sorted(set(a) | set(b)):
        if sym not in a or sym not in b:
            print("only in %s: %s" % ("the first" if sym in a else "the second", sym))
            bad += 1
        elif a[sym] != b[sym]:
            print("differs: %s" % sym)
            bad += 1
    if ka != kb:
        print("kernel symbol lists differ: %s" % sorted(ka ^ kb))
        bad += 1
    print("all identical" if bad == 0 else "%d differences" % bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
