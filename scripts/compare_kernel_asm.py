#!/usr/bin/env python3
"""Compare the bodies of kernels in two `hipcc -S` outputs: compare_kernel_asm.py OLD.s NEW.s SUBSTRING

For every global symbol whose name contains SUBSTRING, the text from its label to its .Lfunc_end label is taken from both files, comments and blank lines
dropped, the function's index taken out of its local labels (.LBB<index>_<n>: the index counts the functions in front, so a kernel added before it
renumbers them), and compared line for line.  Prints one line per kernel that differs or is missing and a summary line; exit status 1 if anything differs.
Used to show that moving a kernel's body (into an .inc, behind `if constexpr`) left its instructions as they were (DESIGN.md sections 3.12 and 3.15)."""
import re
import sys


def bodies(path, sub):
    out, name, cur = {}, None, []
    label = re.compile(r"^([A-Za-z_][\w$.]*):")
    local = re.compile(r"\.LBB\d+_(\d+)")
    for line in open(path, errors="replace"):
        if name is None:
            m = label.match(line)
            if m and sub in m.group(1) and not m.group(1).startswith("."):
                name, cur = m.group(1), []
            continue
        if line.startswith(".Lfunc_end"):
            out[name] = cur
            name = None
            continue
        text = local.sub(r".LBB_\1", line.split(";", 1)[0].rstrip())
        if text.strip():
            cur.append(text)
    return out


def main():
    old, new = bodies(sys.argv[1], sys.argv[3]), bodies(sys.argv[2], sys.argv[3])
    bad = 0
    for k in sorted(set(old) | set(new)):
        if k not in old or k not in new:
            print("only in %s: %s" % ("NEW" if k in new else "OLD", k)); bad += 1
        elif old[k] != new[k]:
            first = next((i for i, (a, b) in enumerate(zip(old[k], new[k])) if a != b), min(len(old[k]), len(new[k])))
            print("differs at line %d (%d / %d lines): %s" % (first, len(old[k]), len(new[k]), k)); bad += 1
    n_lines = sum(len(v) for v in new.values())
    print("%d kernels compared, %d differ or are missing, %d lines of NEW" % (len(set(old) | set(new)), bad, n_lines))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
