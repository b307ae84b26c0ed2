#!/usr/bin/env python3
"""Wait-state check of the DPP operands the compiler cannot see (thorough_dna.hip: fmac_bcast / dpp_rows23_upper are
inline asm, so LLVM's hazard recognizer pads none of their reads).  In every kernel of the built object, a DPP
instruction's src0 must not have been written by a VALU instruction within the 2 preceding wait states, and no
EXEC write may fall within the 5 before it.  Exit status 1 on a finding:
    python profiles/dpp_hazard_check.py"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin/"
# the Newton kernels' objects: the main unit and the two units of the TIPD instantiations
asm = ""
for name in ("thorough_dna.o", "thorough_dna_tipd.o", "thorough_dna_tipd2h.o"):
    obj = os.path.join(ROOT, "epa_ng_amd", "build", name)
    with tempfile.TemporaryDirectory() as d:
        fat, co = os.path.join(d, "fat.bin"), os.path.join(d, "k.co")
        subprocess.check_call([LLVM + "llvm-objcopy", "--dump-section", ".hip_fatbin=" + fat, obj])
        subprocess.check_call([LLVM + "clang-offload-bundler", "--unbundle", "--type=o", "--input=" + fat,
                               "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co])
        asm += subprocess.check_output([LLVM + "llvm-objdump", "-d", co], text=True) + "\n"

def vregs(op):
    m = re.match(r"v\[(\d+):(\d+)\]", op.strip())
    if m:
        return set(range(int(m.group(1)), int(m.group(2)) + 1))
    m = re.match(r"v(\d+)$", op.strip())
    return {int(m.group(1))} if m else set()


ins = []
for l in asm.split("\n"):
    if re.match(r"^[0-9a-f]+ <", l):
        ins.append(None)   # function boundary
        continue
    m = re.match(r"\s+(\S+)\s*(.*?)\s*//", l)
    if m:
        ins.append((m.group(1), m.group(2)))
ndpp = bad = 0
for i, x in enumerate(ins):
    if x is None or "row_newbcast" not in x[1] and "row_ror" not in x[1]:
        continue
    ndpp += 1
    src0 = vregs(x[1].split(",")[1])
    ws, j = 0, i - 1
    while ws < 5 and j >= 0 and ins[j] is not None:
        op, args = ins[j]
        if op == "s_nop":
            ws += int(args.split()[0], 0) + 1
        else:
            dst = args.split(",")[0] if args else ""
            if ws < 2 and op.startswith("v_") and vregs(dst) & src0:
                bad += 1
                print("VGPR write -> DPP read: %s %s  ->  %s %s" % (op, args, x[0], x[1]))
            if "exec" in dst:
                bad += 1
                print("EXEC write -> DPP: %s %s  ->  %s %s" % (op, args, x[0], x[1]))
            ws += 1
        j -= 1
print("row_newbcast / row_ror instructions: %d, unpadded hazards: %d" % (ndpp, bad))
sys.exit(1 if bad else 0)
