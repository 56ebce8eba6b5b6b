"""Instruction count and digest of every function in the device assembly of vislam_ba.hip, to compare two source trees
without a GPU: a refactor that leaves a kernel's machine code alone leaves its line here alone.

    cd mc_slam_amd/csrc && hipcc --offload-arch=gfx950 -O3 -std=c++17 -S --cuda-device-only -o ba.s vislam_ba.hip
    python scripts/kernel_digest.py ba.s              # one line per symbol: name, instructions, sha1 of the stream
    python scripts/kernel_digest.py parent.s new.s    # both side by side, '!=' where they differ

A stream is every instruction line between the symbol's label and its .Lfunc_end, comments, directives and blank lines
stripped, whitespace squeezed; the function number of a basic-block label (.LBB12_3) is dropped, so that a function
added elsewhere does not show as a change here.  Two compiles of one tree give identical output."""
import hashlib, re, sys


def digest(path):
    out, name, ins = {}, None, []
    for line in open(path):
        s = re.sub(r"\.LBB\d+_", ".LBB_", " ".join(line.split(";")[0].split()))
        if name is None:
            m = re.fullmatch(r"([A-Za-z_$][\w$]*):", s)
            if m: name, ins = m.group(1), []
        elif s.startswith(".Lfunc_end"):
            out[name] = (len([i for i in ins if not i.endswith(":")]), hashlib.sha1("\n".join(ins).encode()).hexdigest()[:16])
            name = None
        elif s and (not s.startswith(".") or s.endswith(":")):   # instructions and block labels; no directives
            ins.append(s)
    return out


if __name__ == "__main__":
    tabs = [digest(p) for p in sys.argv[1:3]]
    for k in sorted(set().union(*tabs)):
        cols = ["%6d %s" % t.get(k, (0, "-" * 16)) for t in tabs]
        print(k, *cols, *(["!=" if cols[0] != cols[1] else "=="] if len(cols) == 2 else []))
