"""Per-kernel table from the compiler's own assembly of csrc/attention.hip (hipcc -S --cuda-device-only with the
build's flags): total VGPRs (arch + acc), scratch bytes, occupancy (waves per SIMD), code bytes, and, before the
first s_barrier, the global loads and how many `s_waitcnt vmcnt(0)` (full drains) separate them.

    python tools/r9/attn_asm_table.py attention.s [name-filter-regex]
"""
import re
import subprocess
import sys


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout
        return out.splitlines()
    except (OSError, subprocess.CalledProcessError):
        return names


def main():
    text = open(sys.argv[1]).read()
    pat = re.compile(sys.argv[2]) if len(sys.argv) > 2 else None
    rows = []
    # a kernel runs from its label "<name>:" to the end of the "; Kernel info:" comment block behind it
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?^; Occupancy: \d+)", text, re.M | re.S):
        name, body = m.group(1), m.group(2)
        if "attn_" not in name:
            continue

        def num(key, body=body):
            k = re.search(r"^;\s*" + key + r"\s*[:=]\s*(\d+)", body, re.M)
            return int(k.group(1)) if k else -1

        code = body.split("s_endpgm")[0]
        pre = code.split("s_barrier")[0]
        loads = len(re.findall(r"^\s*(?:global|buffer|flat)_load_", pre, re.M))
        drains = 0
        pending = False
        for line in pre.splitlines():
            if re.match(r"\s*(?:global|buffer|flat)_load_", line):
                pending = True
            elif re.match(r"\s*s_waitcnt\b.*vmcnt\(0\)", line) and pending:
                drains += 1
                pending = False
        rows.append((name, num("NumVgprs") if num("TotalNumVgprs") < 0 else num("TotalNumVgprs"), num("ScratchSize"),
                     num("Occupancy"), num("codeLenInByte"), loads, drains,
                     len(re.findall(r"^\s*s_and_saveexec_b64", pre, re.M))))
    names = demangle([r[0] for r in rows])
    print("| kernel | VGPRs | scratch | occupancy | code bytes | loads before 1st barrier | full drains | exec-masked branches |")
    print("|---|---|---|---|---|---|---|---|")
    for n, r in sorted(zip(names, rows)):
        short = re.sub(r"\(anonymous namespace\)::", "", n)
        short = re.sub(r"^void ", "", short)
        short = re.sub(r"\(.*$", "", short).replace("unsigned short", "u16")
        if pat and not pat.search(short):
            continue
        print("| `" + short + "` | " + " | ".join(str(x) for x in r[1:]) + " |")


if __name__ == "__main__":
    main()
