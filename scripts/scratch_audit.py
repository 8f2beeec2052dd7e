"""Where a kernel's scratch memory goes (r05): per function of a device assembly file (the build keeps them:
soft-grip_amd/build/<hash>/<source>.device.s) the private segment size, the scratch instructions in the prologue / epilogue (callee-saved
registers of a CALLED function: the price of the staged layout) and the scratch instructions inside loops (what could cost time).
usage: python scripts/scratch_audit.py file.device.s [name filter]"""
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "soft-grip_amd"))
import devasm  # noqa: E402

text = open(sys.argv[1]).read()
lines = text.split("\n")
flt = sys.argv[2] if len(sys.argv) > 2 else ""
print("%-58s %9s %8s %10s %10s %9s" % ("function", "bytes/lane", "instr", "scratch ops", "in loops", "in entry/exit"))
for fname, stream in devasm.functions(text).items():
    if not stream or not fname.startswith(("_Z", ".L_Z")) or flt not in fname:
        continue
    # (the compiler's comments say which blocks are loops and, behind the function, its scratch size -- also of a function that is no
    #  kernel, which devasm.kernels does not list: read from the lines themselves, between the stream's first and last line)
    body = lines[stream[0][0] - 1:stream[-1][0]]
    scratch = next((m.group(1) for m in map(re.compile(r";\s*ScratchSize:\s*(\d+)").match, lines[stream[-1][0]:]) if m), "?")
    nscr = nloop = nedge = 0
    nins = 1                       # (the column has always counted the function's own label line)
    inloop, blk = False, 0
    nblocks = sum(1 for l in body if re.match(r"^\.LBB\d+_\d+:", l))
    for l in body:
        if re.match(r"^\.LBB\d+_\d+:", l):
            blk += 1
            inloop = "Loop" in l
            continue
        t = l.strip()
        if "Loop" in l and t.startswith(";"):
            inloop = True
        if not t or t.startswith((";", ".")):
            continue
        nins += 1
        if t.startswith("scratch_") or ("offen" in t and t.startswith("buffer_")):
            nscr += 1
            if inloop:
                nloop += 1
            if blk == 0 or blk == nblocks:
                nedge += 1
    name = subprocess.run(["c++filt", fname.lstrip(".L")], capture_output=True, text=True).stdout.strip()
    name = re.sub(r"\(.*", "", name)
    print("%-58s %9s %8d %10d %10d %9d" % (name[:58], scratch, nins, nscr, nloop, nedge))
