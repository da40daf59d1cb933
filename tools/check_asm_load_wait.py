"""Static check on device assembly (hipcc --cuda-device-only -S file.hip -o file.s): the destination of an inline-asm global load is
not touched — read, copied, spilled or overwritten — before the next inline-asm `s_waitcnt vmcnt`.  The compiler believes such a load
is complete where it is issued, so nothing but register allocation keeps it from copying the register while the data is still on its
way (screen.hip's column form of pass A lost 4 of 86 456 hits that way once, at a loop edge).  The scan is linear in the text of every
kernel whose name contains SUBSTRING: from the load to the first later inline-asm wait.
usage: python tools/check_asm_load_wait.py file.s SUBSTRING"""
import re
import sys


def regs(text):
    out = set()
    for a, b in re.findall(r"\bv\[(\d+):(\d+)\]", text):
        out.update(range(int(a), int(b) + 1))
    out.update(int(a) for a in re.findall(r"\bv(\d+)\b", text))
    return out


def check(path, sub):
    lines = open(path).read().split("\n")
    n_loads, bad, kernels = 0, [], set()
    func, in_asm, pending = None, False, {}      # pending: register -> line of the load it waits for
    for i, l in enumerate(lines):
        t = l.strip()
        m = re.match(r"^(\w+):\s*(;.*)?$", l)
        if m and not l.startswith(".L"):
            func, pending = (m.group(1) if sub in m.group(1) else None), {}
        if func is None or not t or t.startswith((".", ";")) and "ASMSTART" not in t and "ASMEND" not in t:
            continue
        if "ASMSTART" in t:
            in_asm = True
            continue
        if "ASMEND" in t:
            in_asm = False
            continue
        code = t.split(";")[0]
        if in_asm and "s_waitcnt" in code and "vmcnt" in code:
            pending = {}
            continue
        m = re.match(r"global_load_dword\w*\s+(v\d+|v\[\d+:\d+\])\s*,", code) if in_asm else None
        touched = regs(code) & set(pending)
        if m:
            touched -= regs(m.group(1)) - set(pending)
        for r in sorted(touched):
            bad.append("%s: line %d touches v%d, loaded at line %d, before its wait: %s" % (func, i + 1, r, pending[r] + 1, code))
        if m:
            kernels.add(func)
            n_loads += 1
            for r in regs(m.group(1)):
                pending[r] = i
    return n_loads, kernels, bad


if __name__ == "__main__":
    n, kernels, bad = check(sys.argv[1], sys.argv[2])
    for b in bad:
        print(b)
    print("%d inline-asm loads in %d kernels, %d touched before their wait" % (n, len(kernels), len(bad)))
    sys.exit(1 if bad else 0)
