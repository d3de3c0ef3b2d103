"""Is every function of one device assembly file, instruction for instruction, in another?  For changes that add a
defaulted template parameter to the four-chain kernel and must leave every existing instantiation alone.

    python scratch/p4_asm_same.py PARENT.s THIS.s [template argument text the change appends, default ", false"]

Functions are matched by demangled name, with the appended default argument taken off this build's lr_persist4_* names;
inside the bodies block labels lose their function number and symbols are replaced by their (normalised) demangled
names, comments and directives are dropped.  Prints the functions that differ, those only in one file, and a count."""
import re
import subprocess
import sys

parent, this = sys.argv[1], sys.argv[2]
tail = sys.argv[3] if len(sys.argv) > 3 else ", false"


def functions(path):
    out, cur, sym = {}, None, None
    for line in open(path):
        m = re.match(r"^(_Z\w+):\s*(;.*)?$", line)
        if m:
            sym, cur = m.group(1), []
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end"):
            out[sym], cur = cur, None
            continue
        line = line.split(";")[0].rstrip()
        if not line.strip() or re.match(r"^\s*\.(p2align|loc|file|cfi|type|size|section|globl|weak|protected|hidden)", line):
            continue
        cur.append(line)
    return out


def demangle(syms):
    syms = sorted(syms)
    names = subprocess.run(["c++filt"], input="\n".join(syms), capture_output=True, text=True).stdout.split("\n")
    return dict(zip(syms, names))


def norm_name(n, strip):
    if strip and "lr_persist4_" in n:
        n = re.sub(r"(lr_persist4_\w+<[^>(]*)" + re.escape(tail) + ">", r"\1>", n)
    return n


def normalised(path, strip):
    fs = functions(path)
    used = set(fs)
    for body in fs.values():
        for line in body:
            used.update(re.findall(r"_Z\w+", line))
    names = {s: norm_name(n, strip) for s, n in demangle(used).items()}
    out = {}
    for s, body in fs.items():
        text = "\n".join(re.sub(r"_Z\w+", lambda m: "<" + names.get(m.group(0), m.group(0)) + ">", re.sub(r"\.LBB\d+_", ".LBB_", l))
                         for l in body)
        out[names[s]] = text
    return out


a, b = normalised(parent, False), normalised(this, True)
differ = [n for n in a if n in b and a[n] != b[n]]
gone = [n for n in a if n not in b]
new = [n for n in b if n not in a]
for title, lst in (("DIFFERENT", differ), ("ONLY IN " + parent, gone), ("ONLY IN " + this, new)):
    for n in lst:
        print("%s: %s" % (title, n.split("(")[0][-150:]))
print("%d functions of %s: %d identical, %d different, %d missing; %d new in %s" %
      (len(a), parent, len(a) - len(differ) - len(gone), len(differ), len(gone), len(new), this))
sys.exit(1 if differ or gone else 0)
