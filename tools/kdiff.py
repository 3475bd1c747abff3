"""Whether a change left the kernels of one csrc/*.hip alone: python3 tools/kdiff.py tip_unet.hip <another checkout's csrc>
compiles the file from this tree and from the other one to device assembly (build.CFLAGS), splits it at the function labels, drops
comments, directives and blank lines and prints `same` or `DIFF` with both instruction counts per demangled function; exit status 1
on any DIFF.  A comparison of text: equal text is equal code, different text may still be a renamed label."""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from tissue_image_processing_amd import build as b  # noqa: E402

LABEL = re.compile(r"^(_Z\w+|\w+):\s*(;.*)?$")           # a function's label (basic blocks are .LBB..., data sits behind .type @object)


def functions(csrc, name):
    """mangled name -> the instructions of every function of csrc/name"""
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "k.s")
        subprocess.check_call([b._hipcc()] + b.CFLAGS + ["--cuda-device-only", "-S", os.path.join(csrc, name), "-o", asm])
        lines = open(asm).read().splitlines()
    kinds = dict(re.findall(r"^\s*\.type\s+(\S+),@(\w+)", "\n".join(lines), re.M))
    out, cur = {}, None
    for line in lines:
        m = LABEL.match(line)
        if m:
            cur = out.setdefault(m.group(1), []) if kinds.get(m.group(1)) == "function" else None
            continue
        text = line.split(";")[0].strip()
        if cur is not None and text and not text.startswith("."):
            cur.append(text)
    return out


if __name__ == "__main__":
    ours, theirs = functions(b.CSRC, sys.argv[1]), functions(sys.argv[2], sys.argv[1])
    names = sorted(set(ours) | set(theirs))
    nice = subprocess.run(["c++filt"] + names, capture_output=True, text=True).stdout.splitlines()
    diff = 0
    for k, name in zip(names, nice):
        same = ours.get(k) == theirs.get(k)
        diff += not same
        print("%-4s %6d %6d  %s" % ("same" if same else "DIFF", len(ours.get(k, ())), len(theirs.get(k, ())), name[:120]))
    print("%d functions, %d differ" % (len(names), diff))
    sys.exit(1 if diff else 0)
