"""Wait census of the phase kernel's kept device assembly (build_native.device_asm("sg_phase.hip", variant)): how many times a wavefront
issues memory loads and then WAITS for them, and what else in the instruction stream costs it round trips or issue slots.

Per kernel instantiation (the product build), and -- for the profiling build, whose SG_T stamps are visible as reads of the cycle counter --
per interval between two stamps in file order (the compiler keeps the stamps in program order; a loop body is counted once):

  groups     runs "one or more loads -> the first s_waitcnt that waits for that kind" (vector memory: vmcnt, scalar memory: lgkmcnt)
  vmem/flat/smem/lds   load instructions by kind (flat_* loads wait on BOTH counters: the address may be LDS or global)
  div64      fp64 division expansions (v_div_scale_f64 comes in pairs: one per operand)
  sgpr spill v_writelane / v_readlane (an SGPR parked in a VGPR lane)

usage: python scripts/dev/phase_wait_census.py [--prof] [kernel name substring ...]"""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "soft-grip_amd"))
import build_native  # noqa: E402
import devasm  # noqa: E402

STAMP = re.compile(r"^s_mem(real)?time\b")


def census(lines):
    c = dict(groups=0, vmem=0, flat=0, smem=0, lds=0, div64=0, wl=0, rl=0, insts=0, waits=0)
    pend_v = pend_s = False
    for text in lines:
        op = text.split()[0]
        if op.endswith(":"):
            continue
        c["insts"] += 1
        if op.startswith(("global_load", "buffer_load", "scratch_load")):
            c["vmem"] += 1; pend_v = True
        elif op.startswith("flat_load"):
            c["flat"] += 1; pend_v = True
        elif op.startswith(("s_load", "s_buffer_load")):
            c["smem"] += 1; pend_s = True
        elif op.startswith("ds_read") or op.startswith("ds_load"):
            c["lds"] += 1
        elif op == "v_div_scale_f64":
            c["div64"] += 1
        elif op == "v_writelane_b32":
            c["wl"] += 1
        elif op == "v_readlane_b32":
            c["rl"] += 1
        elif op == "s_waitcnt":
            c["waits"] += 1
            if pend_v and "vmcnt" in text:
                c["groups"] += 1; pend_v = False
            if pend_s and "lgkmcnt" in text:
                c["groups"] += 1; pend_s = False
    c["div64"] //= 2
    return c


def fmt(c):
    return ("insts %5d  waits %4d  load->wait groups %3d  vmem %3d  flat %3d  smem %3d  lds %4d  div64 %3d  sgpr spill w/r %3d/%3d"
            % (c["insts"], c["waits"], c["groups"], c["vmem"], c["flat"], c["smem"], c["lds"], c["div64"], c["wl"], c["rl"]))


def main():
    prof = "--prof" in sys.argv
    want = [a for a in sys.argv[1:] if not a.startswith("--")] or ["sg_phase_kernel"]
    text = open(build_native.device_asm("sg_phase.hip", "prof" if prof else "")).read()
    meta = devasm.kernels(text)
    for name, lines in devasm.functions(text).items():
        if not any(w in name for w in want):
            continue
        body = [t for _, t in lines]
        m = meta.get(name)
        print("== %s%s" % (name, "  vgpr %(vgpr)d agpr %(agpr)d sgpr_spill %(sgpr_spill)d vgpr_spill %(vgpr_spill)d scratch %(scratch)d lds %(lds)d" % m if m else ""))
        print("   whole   " + fmt(census(body)))
        if prof:
            cuts = [i for i, t in enumerate(body) if STAMP.match(t)]
            # SG_T0 reads the counter once, every SG_T(k) twice (now, then prev): interval i runs from the last read of one stamp to the
            # first read of the next.  In source order the stamps of sg_phase_env are SG_T(0) 1 2 3 4 24 5 6 7 8 9 (24 sits in the contact loop)
            for k, (a, b) in enumerate(zip(cuts[0::2], cuts[1::2])):
                print("   iv %3d   %s" % (k, fmt(census(body[a + 1:b]))))


if __name__ == "__main__":
    main()
