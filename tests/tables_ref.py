"""The kinematics, dynamics, smooth and point tables restated in Python from the model alone: an independent statement of the layouts
csrc/sg_tables.cpp builds, which tests/test_tables_host.py holds against the builders offset by offset, element by element, exactly.
The host twins do not read them (they run on the builders' own tables: tests/readout_host.py); solve_ref.dof_parents does."""
import numpy as np

from softgrip_amd.mjcf import JNT_FREE, WRAP_JOINT


def kin_dyn_tables(m):
    """the kinematics and dynamics tables as the library lays them out (the sections the header's routines read)"""
    dbl, ints = [], []

    def put(store, arr, dt):
        at = sum(len(x) for x in store)
        store.append(np.ascontiguousarray(arr, dtype=dt).reshape(-1))
        return at

    f, i = np.float64, np.int32
    qa = np.asarray(m.jnt_qposadr)
    ko = dict(nbody=m.nbody, ngeom=0, njnt=m.njnt, nq=m.nq, nlevel=0)
    for name, arr in (("bpos", m.body_pos), ("bquat", m.body_quat), ("jpos", m.jnt_pos), ("jaxis", m.jnt_axis), ("jq0", np.asarray(m.qpos0)[qa])):
        ko[name] = put(dbl, arr, f)
    ko["gpos"] = ko["gmat"] = ko["gsize"] = 0
    for name, arr in (("bpar", m.body_parentid), ("bjadr", m.body_jntadr), ("bjnum", m.body_jntnum), ("jtype", m.jnt_type), ("jqadr", qa)):
        ko[name] = put(ints, arr, i)
    ko["gbody"] = ko["gmeta"] = ko["lstart"] = ko["lbody"] = 0
    order = ["nbody", "ngeom", "njnt", "nq", "nlevel", "bpos", "bquat", "jpos", "jaxis", "jq0", "gpos", "gmat", "gsize", "bpar", "bjadr", "bjnum", "jtype",
             "jqadr", "gbody", "gmeta", "lstart", "lbody"]
    K = (np.array([ko[k] for k in order], i), np.concatenate(dbl), np.concatenate(ints))
    dbl, ints = [], []
    do = dict(nv=m.nv, nsite=m.nsite, ntendon=m.ntendon, nwrap=len(m.wrap_type))
    for name, arr in (("bmass", m.body_mass), ("bipos", m.body_ipos), ("bimat", m.body_imat), ("jspring", np.asarray(m.qpos_spring)[qa]),
                      ("jstiff", m.jnt_stiffness), ("arm", m.dof_armature), ("spos", m.site_pos), ("wprm", m.wrap_prm), ("tstiff", m.tendon_stiffness),
                      ("tspring", m.tendon_lengthspring), ("grav", m.opt_gravity)):
        do[name] = put(dbl, arr, f)
    for name, arr in (("jdof", m.jnt_dofadr), ("sbody", m.site_bodyid), ("tadr", m.tendon_adr), ("tnum", m.tendon_num), ("wtype", m.wrap_type),
                      ("wobj", m.wrap_objid)):
        do[name] = put(ints, arr, i)
    order = ["nv", "nsite", "ntendon", "nwrap", "bmass", "bipos", "bimat", "jspring", "jstiff", "arm", "spos", "wprm", "tstiff", "tspring", "grav", "jdof",
             "sbody", "tadr", "tnum", "wtype", "wobj"]
    Dn = (np.array([do[k] for k in order], i), np.concatenate(dbl), np.concatenate(ints + [np.zeros(1, i)]))
    return K, Dn


def smooth_table(m):
    """the smooth table as the library lays it out (sgs_build), from the model alone"""
    f, i = np.float64, np.int32
    nv, nb = m.nv, m.nbody
    dbody, dpar, last = np.full(nv, -1, i), np.full(nv, -1, i), np.full(nb, -1, i)
    for b in range(1, nb):
        last[b] = last[m.body_parentid[b]]
        for j in range(m.body_jntadr[b], m.body_jntadr[b] + m.body_jntnum[b]):
            for e in range(6 if m.jnt_type[j] == JNT_FREE else 1):
                d = m.jnt_dofadr[j] + e
                dbody[d], dpar[d], last[b] = b, last[b], d
    par = np.asarray(m.body_parentid)
    child = [np.flatnonzero(par[1:] == b) + 1 for b in range(nb)]
    cstart = np.concatenate([[0], np.cumsum([len(c) for c in child])])
    nspatial = sum(int(m.wrap_type[m.tendon_adr[t]] != WRAP_JOINT) for t in range(m.ntendon))
    dbl = [np.asarray(m.dof_damping, f), np.asarray(m.tendon_damping, f), np.asarray(m.actuator_gain, f), np.asarray(m.actuator_bias, f).reshape(-1),
           np.asarray(m.actuator_gear, f)]
    ints = [dbody, dpar, np.asarray(m.actuator_trnid, i), cstart.astype(i), np.concatenate(child + [np.zeros(0, int)]).astype(i)]
    off = [m.nu, nspatial]
    for store in (dbl, ints):
        at = 0
        for arr in store:
            off.append(at)
            at += len(arr)
    return np.array(off, i), np.concatenate(dbl + [np.zeros(1, f)]), np.concatenate(ints + [np.zeros(1, i)])


def point_table(m):
    """the point table as the library lays it out (sgp_build), from the model alone: per body the last dof of its nearest
    ancestor-or-self that has one, per dof the dof before it on the chain"""
    i = np.int32
    nv, nb = m.nv, m.nbody
    own = [[] for _ in range(nb)]
    for b in range(1, nb):
        for j in range(m.body_jntadr[b], m.body_jntadr[b] + m.body_jntnum[b]):
            own[b] += list(range(m.jnt_dofadr[j], m.jnt_dofadr[j] + (6 if m.jnt_type[j] == JNT_FREE else 1)))
    bdof, dpar = np.full(nb, -1, i), np.full(nv, -1, i)
    for b in range(1, nb):
        enter = bdof[m.body_parentid[b]]
        for d in own[b]:
            dpar[d], enter = enter, d
        bdof[b] = enter
    return np.array([0, nb], i), np.concatenate([bdof, dpar, np.zeros(1, i)])
