"""Whether a change left the kernels of one csrc/*.hip alone: python3 tools/kdiff.py [--loop] tip_unet.hip <another checkout's csrc>
compiles the file from this tree and from the other one to device assembly (build.CFLAGS), splits it at the function labels, drops
comments, directives and blank lines and prints `same` or `DIFF` with both instruction counts per demangled function; exit status 1
on any DIFF.  A comparison of text: equal text is equal code, different text may still be a renamed label.

--loop: for a change that moves a matrix kernel's set-up around (other registers everywhere: plain kdiff prints DIFF) and must leave
its hot loop alone.  A function with an MFMA is compared by its OPCODE sequence (the first token of every instruction) between its
first and its last v_mfma; printed are the instruction counts in front of the first MFMA / inside / behind the last one, ours then
theirs, and the first differing opcodes of a loop that differs.  Exit status 1 only when such a loop differs; functions without an
MFMA are compared and printed as above and do not count towards the status."""
import difflib
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


def loop_parts(instrs):
    """(opcodes in front of the first v_mfma, from it to the last one, behind that), or None without an MFMA"""
    ops = [i.split()[0] for i in instrs]
    at = [k for k, o in enumerate(ops) if o.startswith("v_mfma")]
    return (ops[:at[0]], ops[at[0]:at[-1] + 1], ops[at[-1] + 1:]) if at else None


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--loop"]
    loop = len(args) < len(sys.argv) - 1
    ours, theirs = functions(b.CSRC, args[0]), functions(args[1], args[0])
    names = sorted(set(ours) | set(theirs))
    nice = subprocess.run(["c++filt"] + names, capture_output=True, text=True).stdout.splitlines()
    diff = loops = 0
    for k, name in zip(names, nice):
        po, pt = (loop_parts(ours.get(k, ())), loop_parts(theirs.get(k, ()))) if loop else (None, None)
        if po and pt:
            same = po[1] == pt[1]
            loops += not same
            print("%-4s %5d/%5d/%5d %5d/%5d/%5d  %s" % (("same" if same else "DIFF",) + tuple(map(len, po + pt)) + (name[:100],)))
            if not same:
                for line in list(difflib.unified_diff(pt[1], po[1], "theirs", "ours", n=0, lineterm=""))[2:42]:
                    print("       " + line)
        else:
            same = ours.get(k) == theirs.get(k)
            print("%-4s %6d %6d  %s" % ("same" if same else "DIFF", len(ours.get(k, ())), len(theirs.get(k, ())), name[:120]))
        diff += not same
    print("%d functions, %d differ" % (len(names), diff))
    sys.exit(1 if (loops if loop else diff) else 0)
