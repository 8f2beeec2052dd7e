"""Per-dof joint-space forces along one squeeze episode (sg_get_joint_forces): which dof carries the largest passive, bias and actuator
force, step by step -- the companion of scripts/energy_trace.py, which shows THAT an env gains energy; this shows which dof and which
force term is large when it does.

One episode of the reference's 200-step schedule at <= 64 envs with k spread over U(300, 1400).  After the reset and after every env
step, per force term: the largest |entry| over all envs and dofs with its env and dof, and the median over envs of each env's largest
|entry|.  An env that has been flagged stops integrating (sg_step); its later rows repeat the state it stopped in, or are NaN where that
state is not finite, and the statistics leave NaN rows out.

usage: python scripts/force_trace.py --scene softball [--pipeline rows|tree] [--tendon-damper explicit|implicit] [--envs 64] [--seed 0]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# scenes with another layout than the reference's two-finger one: joints / tendons that take the stiffness, actuators
LAYOUT = {"fourfinger_softball": (list(range(65, 283)), [0], 4), "fourfinger_softball_fix": (list(range(65, 283)), [0], 4),
          "freeball": (list(range(9, 227)), [0], 2), "freeball_fix": (list(range(9, 227)), [0], 2)}
TERMS = ("passive", "bias", "actuator")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="softball")
    ap.add_argument("--pipeline", default=None, choices=[None, "rows", "tree"])
    ap.add_argument("--tendon-damper", default="explicit", choices=["explicit", "implicit"])
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--seed", type=int, default=0)
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
    sched = episode_schedule()
    n, T = args.envs, len(sched)
    flags = torch.zeros(n, dtype=torch.int32, device=b.device)
    frc = torch.empty(T + 1, 3, n, nm.nv, dtype=torch.float64, device=b.device)
    fl = torch.zeros(n, T + 1, dtype=torch.int32, device=b.device)

    def read(t):
        f = b.joint_forces()
        for c, name in enumerate(TERMS):
            frc[t, c] = f[name]
        fl[:, t] = flags

    b.reset(1, flags=flags)
    read(0)
    for t, c in enumerate(sched):
        if c is not None:
            b.set_ctrl_broadcast(np.full(nu, c))
        b.step(7, flags=flags)
        read(t + 1)
    frc, fl = frc.cpu().numpy(), fl.cpu().numpy()
    print("# scene %s  pipeline %s  tendon damper %s  envs %d  k in [%.1f, %.1f]  nv %d  (row 0: after sg_reset; row t: after env step t - 1)"
          % (args.scene, args.pipeline or "default", args.tendon_damper, n, ks[0], ks[-1], nm.nv))
    print("# step ctrl flagged " + " ".join("%s_max env dof %s_med" % (x, x) for x in TERMS))
    ctrl, raised = 0.0, np.zeros(n, bool)
    for t in range(T + 1):
        if t > 0 and sched[t - 1] is not None:
            ctrl = sched[t - 1]
        raised |= fl[:, t] != 0
        cells = []
        for c in range(3):
            x = np.abs(frc[t, c])
            ok = np.isfinite(x).all(1)
            if not ok.any():
                cells.append("nan -1 -1 nan")
                continue
            x = np.where(ok[:, None], x, -1.0)
            e, d = np.unravel_index(int(np.argmax(x)), x.shape)
            cells.append("%.6e %2d %3d %.6e" % (x[e, d], e, d, np.median(x[ok].max(1))))
        print("%3d %+.1f %2d %s" % (t, ctrl, int(raised.sum()), " ".join(cells)))
    print("# flagged envs: env k flags step_flagged, then per term the largest |entry| and its dof at the step before the flag")
    for e in np.flatnonzero(raised):
        when = int(np.flatnonzero(fl[e] != 0)[0])
        at = max(when - 1, 0)
        with np.errstate(all="ignore"):
            cells = ["%s %.6e dof %d" % (name, np.nanmax(np.abs(frc[at, c, e])), int(np.nanargmax(np.abs(frc[at, c, e])))) if np.isfinite(frc[at, c, e]).any()
                     else "%s nan" % name for c, name in enumerate(TERMS)]
        print("# %2d %8.2f %2d %3d  %s" % (e, ks[e], int(np.bitwise_or.reduce(fl[e])), when, "  ".join(cells)))
    print("# envs never flagged: %d of %d" % (int((~raised).sum()), n))


if __name__ == "__main__":
    main()
