"""The one reader of the device assembly a build keeps (build_native.device_asm: build/<hash>/<source>.device.s): per kernel its
resource metadata, per function its instruction lines.  Whatever asks the compiler's output a question -- isa_check.py,
scripts/dev/asm_same.py, scripts/scratch_audit.py, the tests that hold a kernel's registers, LDS and scratch -- asks it here."""
import re

# record key -> key of the kernel's entry in the amdhsa.kernels metadata
META = {"vgpr": "vgpr_count", "agpr": "agpr_count", "sgpr_spill": "sgpr_spill_count", "vgpr_spill": "vgpr_spill_count",
        "scratch": "private_segment_fixed_size", "lds": "group_segment_fixed_size"}


def kernels(text):
    """-> {kernel name: {"vgpr", "agpr", "sgpr_spill", "vgpr_spill", "scratch", "lds": int}} (scratch, lds: bytes, the fixed sizes)"""
    out = {}
    for entry in text.split("  - .agpr_count:")[1:]:          # one metadata entry per kernel (its keys are sorted: this one is first)
        entry = ".agpr_count:" + entry
        name = re.search(r"\.name:\s+(\S+)", entry).group(1)
        out[name] = {k: int(re.search(r"\.%s:\s+(\d+)" % key, entry).group(1)) for k, key in META.items()}
    return out


def functions(text):
    """-> {function label: [(line number, text), ...]} in file order: the function's instructions and block labels (.LBB..), comments
    and directives stripped, line numbers from 1.  A whole file names its functions (`.type NAME,@function`) and ends each one
    (.Lfunc_end); in an excerpt without `.type` a function starts at every mangled label (_Z.., .L_Z..) and runs up to the next."""
    declared = set(re.findall(r"^\s*\.type\s+([^\s,]+),@function", text, re.M))
    funcs, cur = {}, None
    for n, line in enumerate(text.split("\n"), 1):
        line = line.split(";", 1)[0].strip()
        m = re.match(r"^([A-Za-z_.][\w$.]*):$", line)
        if m and (m.group(1) in declared if declared else m.group(1).startswith(("_Z", ".L_Z"))):
            cur = funcs.setdefault(m.group(1), [])
        elif line.startswith(".Lfunc_end"):
            cur = None
        elif cur is not None and line and (not line.startswith(".") or re.match(r"^\.LBB\w+:$", line)):
            cur.append((n, line))
    return funcs
