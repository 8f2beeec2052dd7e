"""What the squeeze does to the object: its volume, area, width along a palm-fixed axis, centre of mass and momentum along one episode
(sg_get_shape, sg_get_subtree, sg_get_skin_vertices) next to scripts/contact_force_trace.py's grip force (sg_get_forces).

One episode of the reference's 200-step schedule at <= 64 envs with k spread over U(300, 1400).  After the reset and after every
--every-th env step, medians over the envs that are still running: V and A relative to their values after the reset, dV/dt, the width
hi - lo along --axis given in body --palm's frame (default: the x axis of body 1), the largest displacement of a
skin vertex in the object's frame, the object's centre of mass, its linear momentum M |linvel| and |angmom|, and the summed normal
force between finger geoms and the object.

usage: python scripts/shape_trace.py --scene softbox [--tendon-damper explicit|implicit] [--envs 64] [--seed 0] [--every 10] [--palm 1] [--axis 1,0,0]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from force_trace import LAYOUT  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="softbox")
    ap.add_argument("--tendon-damper", default="explicit", choices=["explicit", "implicit"])
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--every", type=int, default=10)
    ap.add_argument("--palm", type=int, default=1)
    ap.add_argument("--axis", default="1,0,0")
    args = ap.parse_args()
    assert 1 <= args.envs <= 64
    import torch
    import softgrip_amd as sg
    from softgrip_amd import native
    from softgrip_amd.create_dataset import episode_schedule
    jids, tids, nu = LAYOUT.get(args.scene, (list(range(11, 64)), [0], 2))
    m = sg.load_model(os.path.join(ROOT, "models", args.scene + ".sgmodel"), args.tendon_damper)
    nm = native.NativeModel(m)
    nm.set_skin(m.composite_skin())
    b = native.NativeBatch(nm, args.envs, 0)
    ks = np.sort(np.random.RandomState(args.seed).uniform(300, 1400, args.envs))
    b.set_stiffness(ks, jids, tids)
    root, mass = nm.skin_root(), nm.subtree_mass()
    rest = torch.from_numpy(nm.skin_rest(root)).to(b.device)
    axis = np.array([[float(x) for x in args.axis.split(",")]])
    finger = torch.zeros(m.ngeom, dtype=torch.bool, device=b.device)
    finger[[g for g in range(m.ngeom) if m.body_weldid[m.geom_bodyid[g]] != 0 and m.geom_type[g] == 6]] = True
    n, Cn = args.envs, 256
    flags = torch.zeros(n, dtype=torch.int32, device=b.device)
    print("# scene %s  tendon damper %s  envs %d  k in [%.1f, %.1f]  object = body %d (mass %.6g)  skin %d vertices, closed %d  width along (%s) of body %d"
          % (args.scene, args.tendon_damper, n, ks[0], ks[-1], root, mass[root], b.nvert(), nm.skin_closed(), args.axis, args.palm))
    print("# (row 0: after sg_reset; row t: after env step t - 1; medians over the running envs)")
    print("# step ctrl running V/V0 A/A0 dV/dt width max_disp com_x com_y com_z M|linvel| |angmom| grip_N")
    first = {}

    def row(t, ctrl):
        s = b.shape(axis, [args.palm])
        sub = b.subtree()
        local = b.skin_vertices(root, outputs=("local",))["local"]
        f = b.forces(max_rows=1, max_contacts=Cn)
        con = b.contacts(max_contacts=Cn)
        ok = (flags == 0) & (f["ncon"] >= 0)
        if not bool(ok.any()):
            print("%3d %+.1f  0" % (t, ctrl))
            return
        slot = torch.arange(Cn, device=b.device)[None, :] < f["ncon"].clamp(max=Cn)[:, None]
        g = con["geom"].long().clamp(min=0)
        grip = (f["contact_force"][:, :, 0] * (slot & (finger[g[:, :, 0]] ^ finger[g[:, :, 1]]))).sum(1)
        if not first:
            first.update(V=s["shape"][:, 0].clone(), A=s["shape"][:, 1].clone())
        med = lambda x: float(x[ok].double().median())  # noqa: E731
        com = sub["com"][:, root]
        print("%3d %+.1f %2d %.8f %.8f %+.3e %.6f %.3e %.5f %.5f %.5f %.3e %.3e %.4e"
              % (t, ctrl, int(ok.sum()), med(s["shape"][:, 0] / first["V"]), med(s["shape"][:, 1] / first["A"]), med(s["shape"][:, 11]), med((s["hi"] - s["lo"])[:, 0]),
                 med((local - rest).norm(dim=-1).max(dim=-1).values), med(com[:, 0]), med(com[:, 1]), med(com[:, 2]), med(mass[root] * sub["linvel"][:, root].norm(dim=-1)),
                 med(sub["angmom"][:, root].norm(dim=-1)), med(grip)))

    b.reset(1, flags=flags)
    ctrl = 0.0
    row(0, ctrl)
    for t, c in enumerate(episode_schedule()):
        if c is not None:
            ctrl = c
            b.set_ctrl_broadcast(np.full(nu, c))
        b.step(7, flags=flags)
        if (t + 1) % args.every == 0:
            row(t + 1, ctrl)
    print("# envs flagged at the end: %d of %d" % (int((flags != 0).sum()), n))


if __name__ == "__main__":
    main()
