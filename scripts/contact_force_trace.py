"""How hard is it squeezing: the constraint and contact forces along one squeeze episode (sg_get_forces) -- the counterpart of
scripts/force_trace.py, which prints the smooth forces per dof.

One episode of the reference's 200-step schedule at <= 64 envs with k spread over U(300, 1400).  After the reset and after every env
step, over the envs that are still running: the median and the largest ncon, nefc and solver sweeps of the NEXT forward pass; the
summed normal force between finger geoms and the object (every contact with exactly one geom on a finger box, summed per env; median
and largest over the envs); the largest |force| of an equality row and of a limit row with its env.

usage: python scripts/contact_force_trace.py --scene softbox [--pipeline rows|tree] [--tendon-damper explicit|implicit] [--envs 64] [--seed 0] [--every 1]"""
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
    ap.add_argument("--pipeline", default=None, choices=[None, "rows", "tree"])
    ap.add_argument("--tendon-damper", default="explicit", choices=["explicit", "implicit"])
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--every", type=int, default=1)
    args = ap.parse_args()
    assert 1 <= args.envs <= 64
    import torch
    import softgrip_amd as sg
    from softgrip_amd import native
    from softgrip_amd.create_dataset import episode_schedule
    jids, tids, nu = LAYOUT.get(args.scene, (list(range(11, 64)), [0], 2))
    m = sg.load_model(os.path.join(ROOT, "models", args.scene + ".sgmodel"), args.tendon_damper)
    nm = native.NativeModel(m)
    b = native.NativeBatch(nm, args.envs, 0)
    if args.pipeline:
        b.set_pipeline(args.pipeline)
    ks = np.sort(np.random.RandomState(args.seed).uniform(300, 1400, args.envs))
    b.set_stiffness(ks, jids, tids)
    # finger geoms: the moving boxes (the touch words' geoms); a finger - object contact has exactly one of them
    finger = torch.zeros(m.ngeom, dtype=torch.bool, device=b.device)
    finger[[g for g in range(m.ngeom) if m.body_weldid[m.geom_bodyid[g]] != 0 and m.geom_type[g] == 6]] = True
    sched = episode_schedule()
    n, C = args.envs, 256
    flags = torch.zeros(n, dtype=torch.int32, device=b.device)
    print("# scene %s  pipeline %s  tendon damper %s  envs %d  k in [%.1f, %.1f]  nv %d  row capacity %d  (row 0: after sg_reset; row t: after env step t - 1)"
          % (args.scene, args.pipeline or "default", args.tendon_damper, n, ks[0], ks[-1], nm.nv, b.max_rows()))
    print("# step ctrl running ncon_med ncon_max nefc_med nefc_max iters_med iters_max grip_N_med grip_N_max eq_max env limit_max env")

    def row(t, ctrl):
        f = b.forces(max_contacts=C)
        con = b.contacts(max_contacts=C)
        ok = (flags == 0) & (f["nefc"] >= 0)
        if not bool(ok.any()):
            print("%3d %+.1f  0" % (t, ctrl))
            return
        slot = torch.arange(C, device=b.device)[None, :] < f["ncon"].clamp(max=C)[:, None]
        g = con["geom"].long().clamp(min=0)
        grip = (f["contact_force"][:, :, 0] * (slot & (finger[g[:, :, 0]] ^ finger[g[:, :, 1]]))).sum(1)
        rows = torch.arange(f["efc_force"].shape[1], device=b.device)[None, :] < f["nefc"].clamp(min=0)[:, None]
        mag = f["efc_force"].abs() * ok[:, None]
        eq = (mag * (rows & (f["efc_type"] == 0))).max(1).values
        lim = (mag * (rows & (f["efc_type"] == 3))).max(1).values
        sel = lambda x: x[ok].double()  # noqa: E731
        print("%3d %+.1f %2d %5.1f %4d %6.1f %5d %4.1f %3d %.6e %.6e %.6e %2d %.6e %2d"
              % (t, ctrl, int(ok.sum()), float(sel(f["ncon"]).median()), int(sel(f["ncon"]).max()), float(sel(f["nefc"]).median()), int(sel(f["nefc"]).max()),
                 float(sel(f["iters"]).median()), int(sel(f["iters"]).max()), float(sel(grip).median()), float(sel(grip).max()), float(eq.max()), int(eq.argmax()),
                 float(lim.max()), int(lim.argmax())))

    b.reset(1, flags=flags)
    ctrl = 0.0
    row(0, ctrl)
    for t, c in enumerate(sched):
        if c is not None:
            ctrl = c
            b.set_ctrl_broadcast(np.full(nu, c))
        b.step(7, flags=flags)
        if (t + 1) % args.every == 0:
            row(t + 1, ctrl)
    print("# envs flagged at the end: %d of %d" % (int((flags != 0).sum()), n))


if __name__ == "__main__":
    main()
