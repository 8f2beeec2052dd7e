"""Per-env energy along one squeeze episode (sg_get_energy): where an env starts to gain energy, and in which store.

One episode of the reference's 200-step schedule at <= 64 envs with k spread over U(300, 1400).  After the reset and after every env
step: the median and the maximum over envs of the four terms (gravity, joint springs, tendon springs, kinetic) and of their sum; at the
end, for every env that raised a flag, the flag bits, the step at which it raised them and the first step at which its total exceeded
the total it had at reset.  An env that has been flagged stops integrating (sg_step); its later rows repeat the state it stopped in, or
are NaN where that state is not finite, and the statistics leave NaN rows out.

usage: python scripts/energy_trace.py --scene softball [--pipeline rows|tree] [--tendon-damper explicit|implicit] [--envs 64] [--seed 0]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# scenes with another layout than the reference's two-finger one: joints / tendons that take the stiffness, actuators
LAYOUT = {"fourfinger_softball": (list(range(65, 283)), [0], 4), "fourfinger_softball_fix": (list(range(65, 283)), [0], 4),
          "freeball": (list(range(9, 227)), [0], 2), "freeball_fix": (list(range(9, 227)), [0], 2)}
TERMS = ("gravity", "jnt_spring", "ten_spring", "kinetic", "total")


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
    en = torch.empty(n, T + 1, 4, dtype=torch.float64, device=b.device)
    row = torch.empty(n, 4, dtype=torch.float64, device=b.device)
    fl = torch.zeros(n, T + 1, dtype=torch.int32, device=b.device)
    b.reset(1, flags=flags)
    fl[:, 0] = flags
    en[:, 0] = b.energy(out=row)
    for t, c in enumerate(sched):
        if c is not None:
            b.set_ctrl_broadcast(np.full(nu, c))
        b.step(7, flags=flags)
        fl[:, t + 1] = flags
        en[:, t + 1] = b.energy(out=row)
    en, fl = en.cpu().numpy(), fl.cpu().numpy()
    tot = np.concatenate([en, en.sum(2, keepdims=True)], 2)      # [n, T + 1, 5]
    print("# scene %s  pipeline %s  tendon damper %s  envs %d  k in [%.1f, %.1f]  (row 0: after sg_reset; row t: after env step t - 1)"
          % (args.scene, args.pipeline or "default", args.tendon_damper, n, ks[0], ks[-1]))
    print("# step ctrl flagged " + " ".join("%s_med %s_max" % (x, x) for x in TERMS))
    ctrl, raised = 0.0, np.zeros(n, bool)
    with np.errstate(all="ignore"):
        for t in range(T + 1):
            if t > 0 and sched[t - 1] is not None:
                ctrl = sched[t - 1]
            raised |= fl[:, t] != 0
            cells = []
            for c in range(5):
                x = tot[:, t, c]
                x = x[np.isfinite(x)]
                cells.append("%.6e %.6e" % (np.median(x), x.max()) if x.size else "nan nan")
            print("%3d %+.1f %2d %s" % (t, ctrl, int(raised.sum()), " ".join(cells)))
    print("# flagged envs: env k flags step_flagged first_step_total_above_reset total_at_reset total_there")
    for e in np.flatnonzero(raised):
        when = int(np.flatnonzero(fl[e] != 0)[0])
        with np.errstate(all="ignore"):
            above = np.flatnonzero(~(tot[e, :, 4] <= tot[e, 0, 4]))      # (a NaN total counts as above)
        first = int(above[0]) if above.size else -1
        print("# %2d %8.2f %2d %3d %3d %.6e %.6e" % (e, ks[e], int(np.bitwise_or.reduce(fl[e])), when, first, tot[e, 0, 4], tot[e, first, 4] if first >= 0 else np.nan))
    print("# envs never flagged: %d of %d; of those, total above its reset value at the end: %d"
          % (int((~raised).sum()), n, int((tot[~raised, -1, 4] > tot[~raised, 0, 4]).sum())))


if __name__ == "__main__":
    main()
