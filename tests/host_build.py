"""The one g++ build behind every *_ref.build_host: a driver (C++ text) and the csrc files it is built from, in a directory of its own,
with at most one piece of arithmetic replaced -- the builds that show the tests bite -- opened with ctypes."""
import ctypes as C
import os
import shutil
import subprocess

from helpers import ROOT

CSRC = os.path.join(ROOT, "soft-grip_amd", "csrc")


def build(tmpdir, name, driver, copy=(), patch=None, opt="-O2", sources=(), tag="plain"):
    """compiles `driver` into tmpdir/tag/lib<name>.so -> the CDLL.
    copy: csrc files copied beside the driver, so that every include of one of them -- from the driver or from another copy -- finds
    the copy; a .cpp among them is compiled with the driver.  patch: (file of `copy`, old, new), old occurring exactly once.
    sources: further csrc .cpp files compiled as they are"""
    d = os.path.join(str(tmpdir), tag)
    os.makedirs(d, exist_ok=True)
    for f in copy:
        shutil.copy(os.path.join(CSRC, f), os.path.join(d, f))
    if patch is not None:
        which, old, new = patch
        assert which in copy, (which, copy)
        with open(os.path.join(d, which)) as f:
            text = f.read()
        assert text.count(old) == 1, (tag, which, text.count(old))
        with open(os.path.join(d, which), "w") as f:
            f.write(text.replace(old, new))
    src, so = os.path.join(d, name + ".cpp"), os.path.join(d, "lib%s.so" % name)
    with open(src, "w") as f:
        f.write(driver)
    cpp = [os.path.join(d, f) for f in copy if f.endswith(".cpp")] + [os.path.join(CSRC, f) for f in sources]
    subprocess.check_call(["g++", opt, "-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas"] + ["-I", d, "-I", CSRC, "-o", so, src] + cpp)
    return C.CDLL(so)
