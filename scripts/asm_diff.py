"""Per-function diff of two device-assembly listings of one source file (`hipcc --cuda-device-only -S`).

    python scripts/asm_diff.py before.s after.s [--strip-targ ', comms::DecimArgs>=>']

Every function of BEFORE must be in AFTER with the same instructions: labels (.LBB*, .Ltmp*, .Lfunc_end*) are
renumbered in order of appearance and the function's own name is replaced by a placeholder, so that only the
instruction stream is compared.  --strip-targ OLD=>NEW rewrites the demangled names of AFTER before they are matched
(a template parameter appended with a default value changes the mangled names of the existing instantiations).
Prints one line per function of BEFORE and exits 1 if any differs or is missing; functions new in AFTER are listed.
"""
import argparse
import re
import shutil
import subprocess
import sys

FUNC_START = re.compile(r"^(_Z\S+):")
LABEL = re.compile(r"\.L(BB|tmp|func_end|func_begin)[0-9_]+")


def functions(path):
    out, name, body = {}, None, []
    with open(path) as f:
        for line in f:
            m = FUNC_START.match(line)
            if m:
                name, body = m.group(1), []
                continue
            if name is None:
                continue
            body.append(line)
            if line.startswith(".Lfunc_end"):
                out[name] = body
                name = None
    return out


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    res = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True)
    return dict(zip(names, res.stdout.splitlines()))


def normalise(name, body):
    labels = {}

    def sub(m):
        return labels.setdefault(m.group(0), ".L%d" % len(labels))

    lines = []
    for line in body:
        line = line.split(";")[0].rstrip()  # (comments name basic blocks by their global numbers)
        line = line.replace(name, "@F")
        line = LABEL.sub(sub, line)
        if line:
            lines.append(line)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("before")
    ap.add_argument("after")
    ap.add_argument("--strip-targ", action="append", default=[])
    args = ap.parse_args()
    fb, fa = functions(args.before), functions(args.after)
    db, da = demangle(list(fb)), demangle(list(fa))
    rewrites = [r.split("=>", 1) for r in args.strip_targ]
    by_dem = {}
    for mangled, dem in da.items():
        for old, new in rewrites:
            dem = dem.replace(old, new)
        by_dem[dem] = mangled
    bad, matched = 0, set()
    for mangled, body in fb.items():
        other = by_dem.get(db[mangled])
        if other is None:
            print("MISSING  %s" % db[mangled])
            bad += 1
            continue
        matched.add(other)
        a, b = normalise(mangled, body), normalise(other, fa[other])
        same = a == b
        print("%s %6d lines  %s" % ("same   " if same else "DIFFERS", len(a), db[mangled]))
        bad += not same
    for mangled in fa:
        if mangled not in matched:
            print("new      %s" % da[mangled])
    print("%d of %d functions of %s unchanged" % (len(fb) - bad, len(fb), args.before))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
