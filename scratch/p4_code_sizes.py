"""Code size, instruction count and registers of the four-chain kernel's functions in the device assembly the build
keeps (csrc/_build/lr_mcmc-*.s, or the file given): one line per lr_persist4_kernel / lr_persist4_steppers
instantiation.  The difference between a generic and a specialised instantiation of one table size is what sits behind
the configuration switches (and the switches themselves).

    python scratch/p4_code_sizes.py [assembly file] [filter substring]"""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "literate_amd", "csrc", "_build", "lr_mcmc-hip-amdgcn-amd-amdhsa-gfx950.s")
want = sys.argv[2] if len(sys.argv) > 2 else "lr_persist4"

funcs, cur = [], None
for line in open(path):
    m = re.match(r"^(_Z\w+):\s*(;.*)?$", line)
    if m:
        cur = dict(sym=m.group(1), insts=0, valu=0, lds=0, salu=0, branches=0)
        funcs.append(cur)
        continue
    if cur is None:
        continue
    m = re.match(r"^; (codeLenInByte|NumVgprs|ScratchSize)\s*[=:]\s*(\d+)", line)
    if m:
        cur.setdefault(m.group(1), int(m.group(2)))
        if m.group(1) == "ScratchSize":
            cur = None
        continue
    m = re.match(r"^\t([a-z]\w+)", line)
    if m and not line.startswith("\t."):
        op = m.group(1)
        cur["insts"] += 1
        cur["valu"] += op.startswith("v_")
        cur["lds"] += op.startswith("ds_")
        cur["salu"] += op.startswith("s_")
        cur["branches"] += op.startswith("s_cbranch") or op == "s_branch"

funcs = [f for f in funcs if "codeLenInByte" in f]
names = subprocess.run(["c++filt"], input="\n".join(f["sym"] for f in funcs), capture_output=True, text=True).stdout.split("\n")
print("%8s %7s %6s %5s %6s %5s %5s %7s  function" % ("bytes", "insts", "valu", "lds", "salu", "br", "vgpr", "scratch"))
for f, n in zip(funcs, names):
    if want in n:
        print("%8d %7d %6d %5d %6d %5d %5d %7d  %s" % (f["codeLenInByte"], f["insts"], f["valu"], f["lds"], f["salu"], f["branches"],
                                                      f.get("NumVgprs", -1), f.get("ScratchSize", -1), n.split("(")[0][-110:]))
