#!/usr/bin/env python3
"""Per-kernel resource table from the compiler's resource-usage remarks.

Compile the device code with the build's flags plus
    --cuda-device-only -c -Rpass-analysis=kernel-resource-usage
and feed the compiler's stderr to this script (file argument or stdin):

    hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -c \\
        -Rpass-analysis=kernel-resource-usage wukong_amd/csrc/gpu_engine.hip \\
        -o /dev/null 2> remarks.txt
    python tools/kernel_resources.py remarks.txt > table.txt
    python tools/kernel_resources.py --diff parent.txt new.txt

Only the remark's resource lines are read.  CPU only; --diff exits 1 when a
kernel appears or disappears, gains scratch or SGPR spills, or loses
occupancy, and lists every other difference.
"""
import re
import shutil
import subprocess
import sys

FIELDS = [  # (column, remark label)
    ("vgpr", "VGPRs"),
    ("agpr", "AGPRs"),
    ("sgpr", "TotalSGPRs"),
    ("sgpr_spill", "SGPRs Spill"),
    ("vgpr_spill", "VGPRs Spill"),
    ("scratch", "ScratchSize [bytes/lane]"),
    ("lds", "LDS Size [bytes/block]"),
    ("occ", "Occupancy [waves/SIMD]"),
]
LABEL = {label: col for col, label in FIELDS}
REMARK = re.compile(r"remark:\s+(.+?):\s+(\S+)\s+\[-Rpass-analysis=kernel-resource-usage\]")


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if not tool or not names:
        return list(names)
    out = subprocess.run([tool], input="\n".join(names), text=True,
                         capture_output=True, check=True).stdout.split("\n")
    return out[:len(names)]


def short_name(full):
    """`void k<1, 4>(args...)` -> `k<1,4>`: cut the parameter list."""
    depth = 0
    for i, ch in enumerate(full):
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif ch == "(" and depth == 0:
            full = full[:i]
            break
    if full.startswith("void "):
        full = full[5:]
    return full.replace(" ", "")  # one token per name: the table splits on blanks


def parse_remarks(text):
    rows, cur = {}, None
    for line in text.splitlines():
        m = REMARK.search(line)
        if not m:
            continue
        label, value = m.group(1).strip(), m.group(2)
        if label == "Function Name":
            cur = rows.setdefault(value, {})
        elif cur is not None and label in LABEL:
            cur[LABEL[label]] = int(value)
    mangled = sorted(rows)
    table = {}
    for mg, full in zip(mangled, demangle(mangled)):
        name = short_name(full)
        table[mg if name in table else name] = rows[mg]
    return table


def format_table(table):
    cols = [c for c, _ in FIELDS]
    width = max([len(k) for k in table] + [6])
    lines = ["  ".join(["kernel".ljust(width)] + [c.rjust(10) for c in cols])]
    for name in sorted(table):
        lines.append("  ".join([name.ljust(width)] +
                               [str(table[name].get(c, "-")).rjust(10)
                                for c in cols]))
    return "\n".join(lines) + "\n"


def read_table(path):
    with open(path) as f:
        lines = [ln.split() for ln in f if ln.strip()]
    cols = lines[0][1:]
    return {ln[0]: dict(zip(cols, map(int, ln[1:]))) for ln in lines[1:]}


def diff(a_path, b_path):
    a, b = read_table(a_path), read_table(b_path)
    bad = []
    for k in sorted(set(a) ^ set(b)):
        bad.append(f"{k}: only in {a_path if k in a else b_path}")
    for k in sorted(set(a) & set(b)):
        d = {c: (a[k][c], b[k][c]) for c in a[k] if a[k][c] != b[k].get(c)}
        if not d:
            continue
        print(k + ": " + ", ".join(f"{c} {x} -> {y}" for c, (x, y) in d.items()))
        for c, worse in (("scratch", 1), ("sgpr_spill", 1), ("occ", -1)):
            if c in d and (d[c][1] - d[c][0]) * worse > 0:
                bad.append(f"{k}: {c} {d[c][0]} -> {d[c][1]}")
    for msg in bad:
        print("FAIL " + msg)
    print(f"{len(a)} / {len(b)} kernels, {len(bad)} violation(s)")
    return 1 if bad else 0


def main(argv):
    if len(argv) == 4 and argv[1] == "--diff":
        return diff(argv[2], argv[3])
    text = open(argv[1]).read() if len(argv) > 1 else sys.stdin.read()
    sys.stdout.write(format_table(parse_remarks(text)))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
