"""The read-out tables' host builders (csrc/sg_tables.cpp: sgk_build, sgc_from_blob, sgd_build, sgs_build, sgp_build; sg_solve.h: sgv_build)
without a GPU.

  * digests: tests/emu/sg_tables_dump.cpp builds the plans as sg_model_create does and then the six tables, and prints per table its ok flag,
    its err text and a hash of the offset block, of every vector and of the scalars.  tests/golden/readout_table_digests.json holds that
    output for the committed models/*.sgmodel and every tests/data/*.xml the MJCF compiler accepts, in both composite variants; the
    comparison is exact.  The file was recorded when the builders had just moved out of sg_readout.hip, unedited.
  * restatements: a ctypes build of sg_tables.cpp + sg_plan.cpp against the layouts tests/tables_ref.py restates in Python from the
    model alone -- offset by offset, element by element, exactly.
  * refusals: blobs with one array removed or one address moved reach the builders, which answer with their message.
  * scripts/sanitize/host_main.cpp --mutate under ASan + UBSan: every damaged copy of a model through the real builders.

When a table is changed ON PURPOSE, regenerate the digests with
    python tests/test_tables_host.py --regen "<what made it: commit and reason>"
and review the diff of the golden file."""
import ctypes as C
import glob
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

GOLDEN = os.path.join(ROOT, "tests", "golden", "readout_table_digests.json")
CSRC = os.path.join(ROOT, "soft-grip_amd", "csrc")
TABLES = ("kin", "con", "dyn", "smooth", "point", "solve")


# ---- 1. the digests ----
def _digests():
    """label -> the program's line for it, over the whole input set (a scene the MJCF compiler refuses has no line)"""
    emu = os.path.join(ROOT, "tests", "emu")
    subprocess.check_call(["make", "-s", "-C", emu, "sg_tables_dump"])
    inputs = sorted(glob.glob(os.path.join(ROOT, "models", "*.sgmodel"))) + sorted(glob.glob(os.path.join(ROOT, "tests", "data", "*.xml")))
    res = subprocess.run([os.path.join(emu, "sg_tables_dump")] + inputs, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    out = {}
    for line in res.stdout.splitlines():
        label, _, rest = line.partition(": ")
        assert rest and label not in out, line
        if " compile error" not in label:
            out[label] = rest
    return out


def test_tables_match_the_pinned_digests():
    with open(GOLDEN) as f:
        golden = json.load(f)["digests"]
    got = _digests()
    models = {k.rsplit(" ", 1)[0] for k in golden}
    assert len([k for k in models if k.endswith(".sgmodel")]) == 10 and len(golden) == 7 * len(models)      # a plans line and six tables each
    assert all(v.startswith("ok=1 err=''") for k, v in golden.items() if not k.endswith(" plans"))      # (refusals: the tests below)
    assert {v for k, v in golden.items() if k.endswith(" plans")} == {"fast=1 tree=1", "fast=0 tree=1", "fast=0 tree=0"}
    assert sorted(got) == sorted(golden), sorted(set(got) ^ set(golden))
    diff = ["%s\n  pinned: %s\n  now:    %s" % (k, golden[k], got[k]) for k in sorted(got) if got[k] != golden[k]]
    assert not diff, "%d of %d lines changed:\n%s" % (len(diff), len(got), "\n".join(diff))


# ---- 2. the ctypes build of the builders ----
HOST_DRIVER = r"""
#include "sg_readout_host.h"
typedef SgHostTables Tables;
// the tables on the plans as sg_model_create builds them (a blob both refuse: a plan that names no geom)
extern "C" Tables* tables_new(const void* blob, size_t n) {
  Tables* T = new Tables();
  bool fast, tree;
  sg_host_tables_planned(blob, n, T, &fast, &tree);
  return T;
}
extern "C" void tables_free(Tables* T) { delete T; }
template <class H> static int ok_of(const H& h, const char** err) { *err = h.err.c_str(); return h.ok; }
extern "C" int tables_ok(const Tables* T, int t, const char** err) {
  return t == 0 ? ok_of(T->kin, err) : t == 1 ? ok_of(T->con, err) : t == 2 ? ok_of(T->dyn, err) : t == 3 ? ok_of(T->smooth, err)
       : t == 4 ? ok_of(T->point, err) : ok_of(T->solve, err);
}
// part 0: the offset block (ints), 1: the doubles, 2: the ints -> the element count; with out, the elements
template <class O> static long long blk(const O& o, void* out) { if (out) memcpy(out, &o, sizeof o); return sizeof o / 4; }
template <class V> static long long vec(const V& v, void* out) { if (out && !v.empty()) memcpy(out, v.data(), v.size() * sizeof(v[0])); return (long long)v.size(); }
extern "C" long long tables_part(const Tables* T, int t, int part, void* out) {
  if (t == 0) return part == 0 ? blk(T->kin.o, out) : part == 1 ? vec(T->kin.dbl, out) : vec(T->kin.ints, out);
  if (t == 2) return part == 0 ? blk(T->dyn.o, out) : part == 1 ? vec(T->dyn.dbl, out) : vec(T->dyn.ints, out);
  if (t == 3) return part == 0 ? blk(T->smooth.o, out) : part == 1 ? vec(T->smooth.dbl, out) : vec(T->smooth.ints, out);
  if (t == 4) return part == 0 ? blk(T->point.o, out) : part == 1 ? 0 : vec(T->point.ints, out);
  return -1;
}
"""


@pytest.fixture(scope="module")
def hostlib(tmp_path_factory):
    import host_build
    L = host_build.build(tmp_path_factory.mktemp("tables_host"), "tables_host", HOST_DRIVER, opt="-O1", sources=("sg_tables.cpp", "sg_plan.cpp"))
    L.tables_new.restype = C.c_void_p
    L.tables_new.argtypes = [C.c_char_p, C.c_size_t]
    L.tables_free.argtypes = [C.c_void_p]
    L.tables_ok.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_char_p)]
    L.tables_part.restype = C.c_longlong
    L.tables_part.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    return L


def build(L, blob):
    """every table of the blob: name -> dict(ok, err) and, for kin / dyn / smooth / point, off, dbl, ints as arrays"""
    T = L.tables_new(blob, len(blob))
    try:
        out = {}
        for t, name in enumerate(TABLES):
            err = C.c_char_p()
            out[name] = dict(ok=bool(L.tables_ok(T, t, C.byref(err))), err=(err.value or b"").decode())
            if name in ("kin", "dyn", "smooth", "point"):
                for part, (key, dt) in enumerate((("off", np.int32), ("dbl", np.float64), ("ints", np.int32))):
                    a = np.zeros(L.tables_part(T, t, part, None), dt)
                    L.tables_part(T, t, part, a.ctypes.data_as(C.c_void_p))
                    out[name][key] = a
        return out
    finally:
        L.tables_free(T)


def _models(tmpdir):
    """(name, model): the three scenes and two of contacts_ref's random grippers (one of them on a free joint)"""
    import contacts_ref as CR
    import softgrip_amd as sg
    out = [(n, sg.compile_mjcf(os.path.join(ROOT, "tests", "data", n), composite_neighbors=False)) for n in ("mini_gripper.xml", "free_body.xml", "tendon.xml")]
    xmls = CR.sweep_gripper_xmls()
    for g in (0, 1):
        path = os.path.join(str(tmpdir), "tables_g%d.xml" % g)
        with open(path, "w") as f:
            f.write(xmls[g])
        out.append(("gripper %d" % g, sg.compile_mjcf(path, composite_neighbors=False)))
    return out


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    return _models(tmp_path_factory.mktemp("tables_models"))


def _same_padded(got, ref, what):
    """the builder's vector against the restatement's, which may end in one zero of padding the builder leaves out"""
    assert len(ref) - len(got) in (0, 1) and got.dtype == ref.dtype, (what, len(got), len(ref))
    assert got.tobytes() == ref[:len(got)].tobytes() and not ref[len(got):].any(), what


def test_builders_match_the_python_restatements(hostlib, models):
    """the kin sections tables_ref.kin_dyn_tables restates (counts, the body and joint sections of both arrays, which come first), the
    whole dyn table, tables_ref.smooth_table and tables_ref.point_table, exactly.  free_body.xml and the gripper on a free joint carry
    jnt_qposadr / jnt_dofadr.  The geom sections of kin, which kin_dyn_tables leaves at zero, are not compared: the digests hold them"""
    import tables_ref as TR
    kin_names = ["nbody", "ngeom", "njnt", "nq", "nlevel", "bpos", "bquat", "jpos", "jaxis", "jq0", "gpos", "gmat", "gsize", "bpar", "bjadr", "bjnum", "jtype",
                 "jqadr", "gbody", "gmeta", "lstart", "lbody"]
    free = 0
    for name, m in models:
        free += bool(m.has_free_joint)
        got = build(hostlib, m.to_blob())
        for t in ("kin", "dyn", "smooth", "point"):
            assert got[t]["ok"] and not got[t]["err"], (name, t, got[t]["err"])
        (ko, kd, ki), (do, dd, di) = TR.kin_dyn_tables(m)
        o, ro = dict(zip(kin_names, got["kin"]["off"])), dict(zip(kin_names, ko))
        assert len(got["kin"]["off"]) == len(kin_names)
        for k in ("nbody", "njnt", "nq", "bpos", "bquat", "jpos", "jaxis", "jq0", "bpar", "bjadr", "bjnum", "jtype", "jqadr"):
            assert o[k] == ro[k], (name, k, o[k], ro[k])
        assert o["ngeom"] == m.ngeom and o["gpos"] == len(kd) and o["gbody"] == len(ki), name      # the geom sections follow the restated ones
        assert got["kin"]["dbl"][:len(kd)].tobytes() == kd.tobytes() and got["kin"]["ints"][:len(ki)].tobytes() == ki.tobytes(), name
        assert got["dyn"]["off"].tobytes() == do.tobytes(), (name, got["dyn"]["off"], do)
        _same_padded(got["dyn"]["dbl"], dd, (name, "dyn dbl"))
        _same_padded(got["dyn"]["ints"], di, (name, "dyn ints"))
        so, sd, si = TR.smooth_table(m)
        assert got["smooth"]["off"].tobytes() == so.tobytes(), (name, got["smooth"]["off"], so)
        _same_padded(got["smooth"]["dbl"], sd, (name, "smooth dbl"))
        _same_padded(got["smooth"]["ints"], si, (name, "smooth ints"))
        po, pi = TR.point_table(m)
        assert got["point"]["off"].tobytes() == po.tobytes(), (name, got["point"]["off"], po)
        _same_padded(got["point"]["ints"], pi, (name, "point ints"))
    assert free >= 2


# ---- 3. refusals ----
def records(blob):
    """[(name, dtype code, array)] of a blob"""
    nrec, off, out = struct.unpack_from("<I", blob, 8)[0], 24, []
    for _ in range(nrec):
        nm, code, _, cnt = struct.unpack_from("<24sIIq", blob, off)
        dt = {1: np.float64, 2: np.int32, 3: np.uint8}[code]
        out.append((nm.rstrip(b"\0").decode(), code, np.frombuffer(blob, dt, cnt, off + 40).copy()))
        nb = cnt * np.dtype(dt).itemsize
        off += 40 + nb + (-nb) % 8
    assert off == len(blob)
    return out


def pack(recs, head):
    """the blob of the records, under the magic and version of `head` (a blob's first 8 bytes)"""
    body = b""
    for name, code, arr in recs:
        raw = np.ascontiguousarray(arr).tobytes()
        body += struct.pack("<24sIIq", name.encode(), code, 0, arr.size) + raw + b"\0" * ((-len(raw)) % 8)
    magic, ver = struct.unpack("<II", head)
    return struct.pack("<IIIIq", magic, ver, len(recs), 0, len(body) + 24) + body


def damaged(m, drop=None, **put):
    """m's blob without the array `drop` and with the arrays of `put` replaced (or appended, int32, when the blob has none of that name)"""
    blob = m.to_blob()
    recs = [r for r in records(blob) if r[0] != drop]
    for name, arr in put.items():
        at = [i for i, r in enumerate(recs) if r[0] == name]
        if at:
            recs[at[0]] = (name, recs[at[0]][1], np.asarray(arr, recs[at[0]][2].dtype))
        else:
            recs.insert(len(recs) - 1, (name, 2, np.asarray(arr, np.int32)))      # (before `names`, where to_blob puts them)
    return pack(recs, blob[:8])


def _dofadr(m):
    return np.array(m.jnt_dofadr, np.int32)


def _joint_above_joint(m):
    """(a, b): two scalar joints, a on b's body before it or on an ancestor of b's body; None: the model has no such pair"""
    par, jadr, jnum = m.body_parentid, m.body_jntadr, m.body_jntnum
    for body in range(m.nbody - 1, 0, -1):
        mine = [j for j in range(jadr[body], jadr[body] + jnum[body]) if m.jnt_type[j] != 0]
        up = par[body]
        while mine and len(mine) < 2 and up > 0:
            mine = [j for j in range(jadr[up], jadr[up] + jnum[up]) if m.jnt_type[j] != 0][-1:] + mine
            up = par[up]
        if len(mine) >= 2:
            return mine[-2], mine[-1]
    return None


def test_an_intact_blob_survives_the_round_trip(hostlib, models):
    for name, m in models:
        assert damaged(m) == m.to_blob(), name


def test_a_missing_site_quat_is_refused_by_the_point_builder_alone(hostlib, models):
    for name, m in models:
        got = build(hostlib, damaged(m, drop="site_quat"))
        assert got["point"]["err"] == "model blob lacks site_quat" and not got["point"]["ok"], (name, got["point"])
        for t in ("kin", "dyn", "smooth"):
            assert got[t]["ok"], (name, t, got[t]["err"])


def test_every_array_a_builder_reads_is_missed_by_name(hostlib, models):
    """one array removed at a time, every array of the blob: each table either builds or names an array the blob lacks -- the removed
    one, or its own table's refusal passed on"""
    name, m = models[1]
    for rec, _, _ in records(m.to_blob()):
        got = build(hostlib, damaged(m, drop=rec))
        for t in TABLES:
            assert got[t]["ok"] != bool(got[t]["err"]), (rec, t, got[t])
            if not got[t]["ok"] and t != "solve" and rec not in ("jnt_qposadr", "jnt_dofadr"):      # (optional: without them joint j sits at j)
                assert got[t]["err"] == "model blob lacks " + rec, (rec, t, got[t]["err"])


def test_a_dof_address_past_nv_is_refused(hostlib, models):
    for name, m in models:
        adr = _dofadr(m)
        adr[-1] = m.nv
        got = build(hostlib, damaged(m, jnt_dofadr=adr))
        assert got["kin"]["ok"], name
        for t in ("dyn", "smooth", "point"):      # (the dyn table's refusal, passed on)
            assert not got[t]["ok"] and got[t]["err"] == "joint dof address out of range", (name, t, got[t]["err"])


def test_a_dof_order_that_breaks_the_walk_is_refused_by_both_walks(hostlib, models):
    """two joints on one dof; a joint's dofs ahead of its ancestors'; a dof no joint owns (dof_armature and dof_damping one longer):
    the smooth and the point builder each answer with the walk's message, the dyn table builds"""
    ordered = 0
    for name, m in models:
        adr = _dofadr(m)
        cases = [(dict(dof_armature=np.append(m.dof_armature, 0.0), dof_damping=np.append(m.dof_damping, 0.0), jnt_dofadr=adr), "a dof without a joint")]
        if m.njnt >= 2:
            shared = adr.copy()
            shared[-1] = adr[-2]
            cases.append((dict(jnt_dofadr=shared), "two joints share a dof"))
        pair = _joint_above_joint(m)      # (free_body.xml has none: its one joint is the free joint)
        if pair:
            swapped = adr.copy()      # joint b is met below joint a in the walk and now sits on the lower dof
            swapped[pair[0]], swapped[pair[1]] = adr[pair[1]], adr[pair[0]]
            cases.append((dict(jnt_dofadr=swapped), "dofs must follow the order of the bodies and their joints"))
            ordered += 1
        for put, msg in cases:
            got = build(hostlib, damaged(m, **put))
            assert got["dyn"]["ok"], (name, msg, got["dyn"]["err"])
            for t in ("smooth", "point"):
                assert not got[t]["ok"] and got[t]["err"] == msg, (name, t, msg, got[t]["err"])
    assert ordered >= 3      # (tendon.xml has no joint above another either)


# ---- 5. the mutation mode of scripts/sanitize/host_main.cpp ----
def test_sanitizer_run_of_the_builders_over_damaged_blobs(tmp_path):
    """scripts/sanitize/host_main.cpp --mutate -- a stand-alone program: both plan builders and then the six table builders on every damaged
    copy of a blob -- built by g++ with AddressSanitizer and UBSan and run on the CPU: no report, no damaged copy accepted, every builder answers with ok
    or a message.  Three of the ten committed models -- a two-finger one, the four-finger tree and the one on a free joint: with the build, all ten take
    up to a minute (scripts/sanitize/run.sh runs them all)"""
    exe = str(tmp_path / "host_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wno-unknown-pragmas", "-o", exe,
                           os.path.join(ROOT, "scripts", "sanitize", "host_main.cpp")] + [os.path.join(CSRC, s) for s in ("sg_mjcf.cpp", "sg_plan.cpp", "sg_tables.cpp")])
    files = [os.path.join(ROOT, "models", n + ".sgmodel") for n in ("softbox_fix", "fourfinger_softball_fix", "freeball_fix")]
    res = subprocess.run([exe, "--mutate"] + files, capture_output=True, text=True)
    print(res.stdout[-2000:])
    assert res.returncode == 0 and not res.stderr, (res.stdout[-2000:], res.stderr[-4000:])
    assert " 0 accepted" in res.stdout and "SILENT" not in res.stdout and "ACCEPTED" not in res.stdout, res.stdout[-2000:]


if __name__ == "__main__":
    assert len(sys.argv) == 3 and sys.argv[1] == "--regen", __doc__
    digests = _digests()
    with open(GOLDEN, "w") as f:
        json.dump({"header": sys.argv[2], "digests": digests}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d lines -> %s" % (len(digests), GOLDEN))
