"""Static counts of one kernel in a device assembly listing (hipcc -S --cuda-device-only): instructions, the extents of its large
loops (label of a backward branch's target .. the branch), the positions of its s_sleep instructions (the pair waits of
tran_persistent_kernel) and, for an instruction range, the opcodes profiles/r11_notes.md reports.

    python scripts/loop_counts.py device.s 'tran_persistent_kernelILi12ELb1ELi0ELb0' [first last]
"""
import re
import sys
from collections import Counter


def kernel_lines(path, pattern):
    cur, out = None, {}
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = m.group(1)
            out[cur] = []
        elif cur is not None:
            if line.startswith(".Lfunc_end"):
                cur = None
            else:
                out[cur].append(line.rstrip("\n"))
    names = [k for k in out if re.search(pattern, k)]
    assert len(names) == 1, names
    return names[0], out[names[0]]


def instructions(lines):
    """(instructions, position of every .LBB label)"""
    ins, pos = [], {}
    for line in lines:
        t = line.strip()
        m = re.match(r"^(\.LBB\d+_\d+):", t)
        if m:
            pos[m.group(1)] = len(ins)
        elif t and not t.startswith((".", ";", "//")) and not t.endswith(":"):
            ins.append(t)
    return ins, pos


def main():
    name, lines = kernel_lines(sys.argv[1], sys.argv[2])
    ins, pos = instructions(lines)
    print("%s: %d instructions" % (name, len(ins)))
    for i, t in enumerate(ins):
        m = re.match(r"(s_cbranch_\w+|s_branch)\s+(\.LBB\d+_\d+)", t)
        if m and pos.get(m.group(2), len(ins)) <= i and i - pos[m.group(2)] > 2000:
            print("loop %d .. %d: %d instructions" % (pos[m.group(2)], i, i - pos[m.group(2)] + 1))
    print("s_sleep at", [i for i, t in enumerate(ins) if t.startswith("s_sleep")])
    if len(sys.argv) > 4:
        seg = ins[int(sys.argv[3]):int(sys.argv[4]) + 1]
        c = Counter(t.split()[0] for t in seg)
        exec_writes = sum(1 for t in seg if re.match(r"s_\w+\s+exec\b", t) or "saveexec" in t.split()[0])
        print("range: %d instructions, v_readlane %d, saveexec %d, exec writes %d, v_cndmask %d, v_fma_f64 %d, v_mov_b64_dpp %d" % (
            len(seg), c["v_readlane_b32"], sum(v for k, v in c.items() if "saveexec" in k), exec_writes,
            sum(v for k, v in c.items() if k.startswith("v_cndmask")), c["v_fma_f64"], c["v_mov_b64_dpp"]))


if __name__ == "__main__":
    main()
