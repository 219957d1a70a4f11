#!/usr/bin/env python3
"""device code of HIP sources in another checkout of this project against this tree, kernel by kernel: the rows of
tools/kernel_resources.py and the instruction stream (hipcc with the build's flags, --cuda-device-only -S; comments, directives and
the numbering of local labels left out).  For changes that must leave kernels alone.  Needs no GPU.
   python tools/device_code_diff.py /path/to/other/checkout odam_amd/csrc/conv_gemm.hip odam_amd/csrc/cg_big_f32.hip ... > table.txt"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
from __graft_entry__ import COMPILE_FLAGS, HIPCC, PER_FILE_FLAGS  # noqa: E402


def resources(tree, rel):
    out = subprocess.run([sys.executable, os.path.join(HERE, "tools", "kernel_resources.py"), os.path.join(tree, rel)] +
                         list(PER_FILE_FLAGS.get(os.path.basename(rel), ())), capture_output=True, text=True).stdout.splitlines()[1:]
    return {ln[40:].strip(): " ".join(ln[:40].split()) for ln in out}      # name (cut at 150 characters) -> VGPR AGPR SGPR spill scratch occupancy


def streams(tree, rel, tmp, tag):
    s = os.path.join(tmp, "%s_%s.s" % (tag, os.path.basename(rel)))
    subprocess.check_call([HIPCC] + COMPILE_FLAGS + list(PER_FILE_FLAGS.get(os.path.basename(rel), ())) +
                          ["--cuda-device-only", "-S", os.path.join(tree, rel), "-o", s], stderr=subprocess.DEVNULL)
    txt = open(s).read()
    out = {}
    for m in re.finditer(r"^(_Z\w+):\s*; @\1\n(.*?)^\.Lfunc_end\d+:", txt, re.S | re.M):
        if ".amdhsa_kernel " + m.group(1) not in txt:
            continue
        ins = []
        for ln in m.group(2).splitlines():
            ln = ln.split(";")[0].strip()
            if ln and (not ln.startswith(".") or ln.endswith(":")):
                ins.append(re.sub(r"\.LBB\d+_", ".LBB_", ln))
        out[subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip()] = ins
    return out


def main(other, files):
    with tempfile.TemporaryDirectory() as tmp:
        jobs = [(tree, rel, tag) for rel in files for tree, tag in ((other, "other"), (HERE, "this"))]
        with ThreadPoolExecutor(max_workers=min(6, os.cpu_count() or 1)) as ex:
            got = dict(zip([(tag, rel) for _, rel, tag in jobs], ex.map(lambda j: (resources(j[0], j[1]), streams(j[0], j[1], tmp, j[2])), jobs)))
    total = same = 0
    print("%-18s %-68s %6s %6s  %-12s %-12s  %-20s %-20s  %s" % ("file", "kernel", "instr", "instr", "sha256", "sha256", "V A S spill scr occ", "V A S spill scr occ", "verdict"))
    for rel in files:
        (ro, so), (rt, st) = got["other", rel], got["this", rel]
        for name in sorted(set(so) | set(st)):
            a, b = so.get(name), st.get(name)
            ha, hb = (hashlib.sha256("\n".join(x).encode()).hexdigest()[:12] if x is not None else "-" for x in (a, b))
            ok = a is not None and a == b and ro.get(name[:150]) == rt.get(name[:150])
            total += 1; same += ok
            short = re.sub(r"^void (odam_\w+::)?|\(odam_\w+::\w+\)$", "", name)
            print("%-18s %-68s %6s %6s  %-12s %-12s  %-20s %-20s  %s" % (os.path.basename(rel), short[:68], len(a) if a is not None else "-", len(b) if b is not None else "-",
                                                                         ha, hb, ro.get(name[:150], "-"), rt.get(name[:150], "-"), "identical" if ok else "DIFFERS"))
    print("%d kernels, %d identical (the other checkout's column first)" % (total, same))
    return 0 if total == same else 1


if __name__ == "__main__":
    sys.exit(main(os.path.abspath(sys.argv[1]), sys.argv[2:]))
