"""Tabulate the compiler's resource report of the kernels whose names match a pattern.

    python -m pycmf_amd.build --force --verbose > build.log 2>&1
    python tools/kernel_resources.py build.log [other.log] [--match als_]

Reads the remarks of -Rpass-analysis=kernel-resource-usage (what ``pycmf_amd.build --verbose`` asks for) and prints one markdown
row per kernel instance: VGPRs, AGPRs, SGPRs, scratch bytes per lane, LDS bytes and waves per SIMD.  With a second log (a build of
another commit) the two are printed side by side and the instances that differ are marked.  Needs no GPU."""
import re
import subprocess
import sys

FIELDS = (("VGPRs", "VGPRs"), ("AGPRs", "AGPRs"), ("TotalSGPRs", "SGPRs"), ("ScratchSize [bytes/lane]", "scratch"),
          ("LDS Size [bytes/block]", "LDS"), ("Occupancy [waves/SIMD]", "waves/SIMD"))


def parse(path):
    out, cur = {}, None
    with open(path, errors="replace") as f:
        for line in f:
            m = re.search(r"remark: Function Name: (\S+)", line)
            if m:
                cur = out.setdefault(m.group(1), {})
                continue
            if cur is None:
                continue
            for key, name in FIELDS:
                m = re.search(r"remark:\s+%s: (\d+)" % re.escape(key), line)
                if m:
                    cur[name] = int(m.group(1))
    return out


def demangle(names):
    try:
        res = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return dict(zip(names, res))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def short(name):
    name = re.sub(r"^void ", "", name)
    name = re.sub(r"\(.*$", "", name)
    return name.replace("cmfk::", "")


def main(argv):
    match = "als_"
    if "--match" in argv:
        i = argv.index("--match")
        match = argv[i + 1]
        argv = argv[:i] + argv[i + 2:]
    logs = [parse(p) for p in argv]
    if not logs:
        sys.exit(__doc__)
    names = [n for n in logs[0] if match in n]
    pretty = demangle(names)
    # an added kernel argument changes the mangled name: instances are paired by their demangled name without the argument list
    other = {}
    if len(logs) > 1:
        opretty = demangle(list(logs[1]))
        other = {short(opretty[n]): v for n, v in logs[1].items()}
    cols = [name for _, name in FIELDS]
    print("| kernel | " + " | ".join(cols) + " |" + (" differs |" if other else ""))
    print("|---|" + "---|" * (len(cols) + (1 if other else 0)))
    for n in sorted(names, key=lambda n: pretty[n]):
        a, key = logs[0][n], short(pretty[n])
        if other:
            # a kernel that gained a trailing bool template argument pairs its `false` instance with the old kernel
            b = other.get(key, other.get(re.sub(r"(, |<)false>$", lambda m: ">" if m.group(1) == ", " else "", key)))
            cells = ["%s / %s" % (a.get(c, "?"), "-" if b is None else b.get(c, "?")) for c in cols]
            diff = "new" if b is None else ", ".join(c for c in cols if a.get(c) != b.get(c))
            print("| %s | %s | %s |" % (key, " | ".join(cells), diff))
        else:
            print("| %s | %s |" % (key, " | ".join(str(a.get(c, "?")) for c in cols)))


if __name__ == "__main__":
    main(sys.argv[1:])
