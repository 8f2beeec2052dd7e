"""soft-grip_amd/build_native.py without a compiler -- the lock, the second look at what is stale, the variant table and the finders of
the kept assembly -- and soft-grip_amd/devasm.py on hand-written text.  build_native is pointed at a directory of the test's own (its
path globals; in the child processes by assignment) and _compile_locked is a stub that logs when it is entered and left, sleeps 0.3 s
and touches the library: nothing here compiles, and nothing touches the checkout's own build/."""
import os
import subprocess
import sys
import time

import pytest

from helpers import ROOT
from test_isa_guard import BAD

PKG = os.path.join(ROOT, "soft-grip_amd")
DRIVER = '''
import os, sys, threading, time
sys.path.insert(0, %r)
import build_native as b
root, mode = sys.argv[1], sys.argv[2]
b._HERE, b.CSRC = root, os.path.join(root, "csrc")

def log(word):
    fd = os.open(os.path.join(root, "log"), os.O_WRONLY | os.O_APPEND | os.O_CREAT)
    os.write(fd, ("%%s %%.6f %%d %%d\\n" %% (word, time.time(), os.getpid(), threading.get_ident())).encode())
    os.close(fd)

def stub(out, extra, verbose, sources, default_sched):
    log("enter")
    time.sleep(0.3)
    open(out, "w").close()
    log("exit")
    return out

b._compile_locked = stub
if mode == "threads":
    ts = [threading.Thread(target=b.build, kwargs=dict(force=True)) for _ in range(2)]
    [t.start() for t in ts]
    [t.join() for t in ts]
else:
    if "wait" in sys.argv:                      # start together: say ready, go when the test says so
        open(os.path.join(root, "ready.%%d" %% os.getpid()), "w").close()
        while not os.path.exists(os.path.join(root, "go")):
            time.sleep(0.002)
    print(b.build(force=mode == "force"))
''' % PKG


@pytest.fixture
def tree(tmp_path):
    """a directory with what needs_build looks at: the sources (empty files) and no library"""
    from softgrip_amd import build_native
    (tmp_path / "csrc").mkdir()
    for s in build_native.VARIANTS["legacy"].sources + ["sg_kernels.hip"]:
        (tmp_path / "csrc" / s).write_text("")
    (tmp_path / "driver.py").write_text(DRIVER)
    return tmp_path


def child(tree, *args):
    return subprocess.Popen([sys.executable, str(tree / "driver.py"), str(tree)] + list(args), stdout=subprocess.PIPE, text=True)


def finish(procs):
    outs = [p.communicate(timeout=60)[0].strip() for p in procs]
    assert [p.returncode for p in procs] == [0] * len(procs)
    return outs


def log_of(tree):
    return [(w, float(t), int(pid), int(tid)) for w, t, pid, tid in (line.split() for line in (tree / "log").read_text().splitlines())]


def wait_for(cond):
    t0 = time.time()
    while not cond():
        assert time.time() - t0 < 30
        time.sleep(0.005)


def assert_no_overlap(log, n):
    """n builders went through the stub, one after the other: in the order of the log every `enter` is followed by its own `exit`"""
    assert [w for w, _, _, _ in log] == ["enter", "exit"] * n, log
    for a, b in zip(log[0::2], log[1::2]):
        assert a[2:] == b[2:] and a[1] <= b[1], log
    assert all(b[1] <= c[1] for b, c in zip(log[1::2], log[2::2])), log


def test_two_threads_of_one_process_do_not_build_together(tree):
    finish([child(tree, "threads")])
    log = log_of(tree)
    assert_no_overlap(log, 2)
    assert len({tid for _, _, _, tid in log}) == 2


def test_a_build_that_starts_during_a_forced_one_waits(tree):
    """A removes the object cache and compiles under one hold of the lock; B, started while A is in the compiler, waits at the same lock
    file (it is outside what A removed) and then finds A's library up to date"""
    a = child(tree, "force")
    wait_for(lambda: (tree / "log").exists())
    b = child(tree, "build")
    outs = finish([a, b])
    assert outs[0] == outs[1] == str(tree / "libsoftgrip.so")
    assert_no_overlap(log_of(tree), 1)


def test_builders_that_waited_at_one_lock_stay_one_at_a_time_after_a_forced_build(tree):
    """X compiles; A (forced) and B arrive while it does, so both wait at the lock X holds.  Whoever goes next, the lock is still the
    one file -- a forced removal does not hand the other one a lock of its own -- and B, forced to nothing, finds the library made"""
    x = child(tree, "build")
    wait_for(lambda: (tree / "log").exists())
    a, b = child(tree, "force"), child(tree, "build")
    assert len(set(finish([x, a, b]))) == 1
    assert_no_overlap(log_of(tree), 2)        # X and A


def test_of_four_processes_on_a_stale_library_one_builds(tree):
    lib = tree / "libsoftgrip.so"
    lib.write_text("")
    os.utime(lib, (time.time() - 1000,) * 2)                    # older than its sources
    procs = [child(tree, "build", "wait") for _ in range(4)]
    wait_for(lambda: len(list(tree.glob("ready.*"))) == 4)
    (tree / "go").write_text("")
    assert finish(procs) == [str(lib)] * 4
    assert_no_overlap(log_of(tree), 1)


@pytest.mark.parametrize("variant", ["", "prof", "count", "legacy"])
def test_the_finders_look_where_the_variant_is_compiled(tree, monkeypatch, variant):
    from softgrip_amd import build_native as b
    seen = []
    monkeypatch.setattr(b, "_HERE", str(tree))
    monkeypatch.setattr(b, "CSRC", str(tree / "csrc"))
    monkeypatch.setattr(b, "_compile_locked", lambda *a: seen.append(a) or a[0])
    assert b.build(**({variant: True} if variant else {})) == str(tree / b.VARIANTS[variant].lib)
    (out, extra, verbose, sources, default_sched), = seen
    assert out == str(tree / b.VARIANTS[variant].lib) and not verbose
    assert ("sg_legacy.hip" in sources) == (variant == "legacy") and set(b.SOURCES) <= set(sources)
    objdir = tree / "build" / b._objdir_name(extra, default_sched)          # where _compile_locked puts objects and assembly
    objdir.mkdir(parents=True)
    assert b.device_asm_files(variant) == []
    with pytest.raises(FileNotFoundError, match="nope.hip"):
        b.device_asm("nope.hip", variant)
    for name in ("sg_tree.device.s", "sg_api.device.s"):
        (objdir / name).write_text("")
    assert b.device_asm_files(variant) == [str(objdir / "sg_api.device.s"), str(objdir / "sg_tree.device.s")]
    assert b.device_asm("sg_tree.hip", variant) == str(objdir / "sg_tree.device.s")
    # one rule for "nothing is stale", whichever the variant: the library is there and newer than its sources -> no compile
    (tree / b.VARIANTS[variant].lib).write_text("")
    b.build(**({variant: True} if variant else {}))
    assert len(seen) == 1


def test_the_variant_directories_differ_and_keep_their_formula():
    from softgrip_amd import build_native as b
    import hashlib
    names = {v: b._objdir_name(e.extra, e.default_sched) for v, e in b.VARIANTS.items()}
    assert len(set(names.values())) == 4 and b.OWNED_VARIANTS == ("prof", "count", "legacy")
    # (an object cache made before stays valid: flags, extra flags, default-scheduler sources, then the per-source flags)
    key = b.FLAGS + ["-DSG_SECTION_PROF", "sg_phase.hip"] + ["%s:%s" % (k, " ".join(v)) for k, v in sorted(b.SOURCE_FLAGS.items())]
    assert names["prof"] == hashlib.sha1(" ".join(key).encode()).hexdigest()[:12]


META_TEXT = """
amdhsa.kernels:
  - .agpr_count:     3
    .args:
      - .offset:         0
        .size:           8
    .group_segment_fixed_size: 256
    .name:           _Z5firstPd
    .private_segment_fixed_size: 0
    .sgpr_count:     20
    .sgpr_spill_count: 0
    .symbol:         _Z5firstPd.kd
    .vgpr_count:     61
    .vgpr_spill_count: 0
  - .agpr_count:     0
    .group_segment_fixed_size: 21392
    .name:           second
    .private_segment_fixed_size: 1632
    .sgpr_count:     104
    .sgpr_spill_count: 12
    .vgpr_count:     128
    .vgpr_spill_count: 7
amdhsa.target:   amdgcn-amd-amdhsa--gfx950
"""


def test_devasm_kernels():
    from softgrip_amd import devasm
    assert devasm.kernels(META_TEXT) == {
        "_Z5firstPd": dict(vgpr=61, agpr=3, sgpr_spill=0, vgpr_spill=0, scratch=0, lds=256),
        "second": dict(vgpr=128, agpr=0, sgpr_spill=12, vgpr_spill=7, scratch=1632, lds=21392)}
    assert devasm.kernels(BAD) == {}


def test_devasm_functions_on_handwritten_assembly():
    from softgrip_amd import devasm
    assert devasm.functions(BAD) == {"_Z6kernelv": [
        (3, ".LBB0_1:"), (4, "v_add_f64 v[0:1], v[0:1], v[2:3]"), (5, "s_andn2_b64 exec, exec, s[4:5]"), (6, "s_cbranch_execz .LBB0_3"),
        (7, "s_branch .LBB0_1"), (8, ".LBB0_3:"), (9, "v_readlane_b32 s0, v255, 3"), (10, "v_accvgpr_write_b32 a0, v6"),
        (11, "s_mov_b32 s88, s78"), (12, "s_or_b64 exec, exec, s[0:1]"), (13, "v_add_f64 v[4:5], v[0:1], v[6:7]"), (14, "s_endpgm")]}
    # a whole file says which labels are functions and where each ends; what lies between two functions belongs to neither
    whole = "\t.type\t_Z1fv,@function\n_Z1fv: ; @_Z1fv\n; %bb.0:\n\ts_nop 0 ; a comment\n\t.p2align 6\n.LBB0_1:\n\ts_endpgm\n.Lfunc_end0:\n" \
            "\t.type\ttable,@object\ntable:\n\t.long 1\n_Z5strayv:\n\ts_nop 1\n\t.type\tg,@function\ng:\n\ts_setpc_b64 s[30:31]\n.Lfunc_end1:\n"
    assert devasm.functions(whole) == {"_Z1fv": [(4, "s_nop 0"), (6, ".LBB0_1:"), (7, "s_endpgm")], "g": [(16, "s_setpc_b64 s[30:31]")]}


def test_devasm_functions_on_the_excerpt():
    """no .type directive, no .Lfunc_end: the mangled label opens the function, and the flagged block is in it"""
    from softgrip_amd import devasm
    with open(os.path.join(ROOT, "tests", "data", "tree_mono_d03dd81_site.s")) as f:
        funcs = devasm.functions(f.read())
    (name, body), = funcs.items()
    assert name.startswith("_Z14sg_tree_kernelILi24E")
    assert ".LBB16_1313:" in [t for _, t in body] and body[0] == (6, "s_mov_b64 exec, s[4:5]")
