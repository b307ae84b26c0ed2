#!/usr/bin/env python3
"""Device assembly of the HIP sources, kernel by kernel, at two commits.

  asm_compare.py emit OUTDIR [file.hip ...]   gfx950 assembly of the sources (default: all of DEV_SOURCES that exist),
                                              with the flags of epa_ng_amd/build.py + --cuda-device-only -S
  asm_compare.py compare DIR_A DIR_B          every kernel of DIR_A must be in DIR_B with the same text

A kernel is the text between its label and its .Lfunc_end plus its .amdhsa_kernel block, keyed by the mangled name;
the union is taken over all .s files of a directory, so a kernel may move between files (and be present twice).  The
per-file function index of local labels and the __hip_cuid_<hash> symbol are normalised first.  Run `emit` in a checkout
of each commit, then `compare` the two directories; exit status 1 on any difference.
"""
import importlib.util
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def emit(outdir, files):
    spec = importlib.util.spec_from_file_location("epa_build", os.path.join(ROOT, "epa_ng_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    os.makedirs(outdir, exist_ok=True)
    procs = []
    for src in files or [s for s in b.DEV_SOURCES if os.path.exists(os.path.join(b.CSRC, s))]:
        cmd = [b.HIPCC] + b.DEV_FLAGS + b.EXTRA_FLAGS.get(src, []) + ["--cuda-device-only", "-S", os.path.join(b.CSRC, src),
                                                                      "-o", os.path.join(outdir, src.replace(".hip", ".s"))]
        procs.append((src, subprocess.Popen(cmd, stderr=subprocess.DEVNULL)))
    bad = [src for src, p in procs if p.wait() != 0]
    if bad:
        sys.exit("hipcc failed on " + " ".join(bad))


def kernels(d):
    """mangled name -> set of normalised texts (one per file that defines the kernel)"""
    out = {}
    for f in sorted(os.listdir(d)):
        if not f.endswith(".s"):
            continue
        text = open(os.path.join(d, f)).read()
        text = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_X", text)
        text = re.sub(r"BB\d+_", "BBn_", text)       # .LBB<k>_<i> labels and the BB<k>_<i> of the loop comments
        text = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1n", text)
        text = re.sub(r"\.Ltmp\d+", ".Ltmpn", text)
        text = re.sub(r"[ \t]+;", " ;", text)          # the comment column moves with the index's digits
        for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)\n.*?^\s*\.end_amdhsa_kernel", text, re.M | re.S):
            name = m.group(1)
            body = re.search(r"^%s:.*?^\.Lfunc_endn:" % re.escape(name), text, re.M | re.S)
            if not body:
                sys.exit("%s: no body of %s" % (f, name))
            out.setdefault(name, set()).add(body.group(0) + "\n" + m.group(0))
    return out


def compare(a, b):
    ka, kb = kernels(a), kernels(b)
    missing = sorted(set(ka) - set(kb))
    differ = sorted(n for n in ka if n in kb and ka[n] != kb[n])
    for n in missing:
        print("missing in %s: %s" % (b, n))
    for n in differ:
        print("differs: %s" % n)
    print("%d kernels in %s, %d in %s (%d new): %d missing, %d differ"
          % (len(ka), a, len(kb), b, len(set(kb) - set(ka)), len(missing), len(differ)))
    return 1 if missing or differ else 0


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "emit":
        emit(sys.argv[2], sys.argv[3:])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
