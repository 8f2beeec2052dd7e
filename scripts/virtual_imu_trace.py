"""What would an IMU read somewhere else on the same link?  One scene, a short squeeze: per env step the accelerometer and gyro magnitude
at the model's own IMU sites next to a few alternative placements on the same bodies -- the body frame's origin and the site moved by
+-`--shift` metres along each body axis -- without touching the model (sg_get_point_motion).

Every env step is taken as the header's recipe takes it: sg_step(n - 1), qpos and qvel copied out, sg_step(1), then the point read-out
at the copied state with that substep's qacc (qacc_warmstart), so the readings belong to the same forward pass as the step's
sensordata; the first column block checks that: the largest deviation of the virtual readings at the model's own sites from it.
Magnitudes are medians over the envs.

usage: python scripts/virtual_imu_trace.py [--scene softbox] [--steps 20] [--envs 16] [--shift 0.02] [--tendon-damper explicit|implicit] [--seed 0]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# scenes with another layout than the reference's two-finger one: joints / tendons that take the stiffness, actuators
LAYOUT = {"fourfinger_softball": (list(range(65, 283)), [0], 4), "fourfinger_softball_fix": (list(range(65, 283)), [0], 4),
          "freeball": (list(range(9, 227)), [0], 2), "freeball_fix": (list(range(9, 227)), [0], 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="softbox")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--envs", type=int, default=16)
    ap.add_argument("--shift", type=float, default=0.02)
    ap.add_argument("--substeps", type=int, default=7)
    ap.add_argument("--tendon-damper", default="explicit", choices=["explicit", "implicit"])
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    assert 1 <= args.envs <= 64 and args.substeps >= 1
    import torch
    import softgrip_amd as sg
    from softgrip_amd import native
    from softgrip_amd.mjcf import SENS_ACCELEROMETER, SENS_GYRO
    jids, tids, nu = LAYOUT.get(args.scene, (list(range(11, 64)), [0], 2))
    m = sg.load_model(os.path.join(ROOT, "models", args.scene + ".sgmodel"), args.tendon_damper)
    nm = native.NativeModel(m)
    b = native.NativeBatch(nm, args.envs, 0)
    ks = np.sort(np.random.RandomState(args.seed).uniform(300, 1400, args.envs))
    b.set_stiffness(ks, jids, tids)
    body, pos, quat = nm.sites()
    chan = {}      # site -> {kind: sensordata address}
    for s in range(len(m.sensor_type)):
        if int(m.sensor_type[s]) in (SENS_ACCELEROMETER, SENS_GYRO):
            chan.setdefault(int(m.sensor_objid[s]), {})["accel" if int(m.sensor_type[s]) == SENS_ACCELEROMETER else "gyro"] = int(m.sensor_adr[s])
    imu = sorted(chan)
    shifts = [("site", None)] + [("origin", "origin")] + [("%s%s" % (sgn, ax), (k, sg_)) for k, ax in enumerate("xyz") for sgn, sg_ in (("+", 1.0), ("-", -1.0))]
    pb, pp, pq = [], [], []
    for s in imu:
        for _, how in shifts:
            p = pos[s].copy()
            if how == "origin":
                p[:] = 0.0
            elif how is not None:
                p[how[0]] += how[1] * args.shift
            pb.append(body[s]); pp.append(p); pq.append(quat[s])
    pb, pp, pq = np.array(pb, np.int32), np.array(pp), np.array(pq)
    n, P = args.envs, len(shifts)
    sens = torch.zeros(n, nm.nsensordata, dtype=torch.float64, device=b.device)
    flags = torch.zeros(n, dtype=torch.int32, device=b.device)
    b.reset(1, sens=sens, flags=flags)
    b.set_ctrl_broadcast(np.full(nu, -0.2))
    print("# scene %s  tendon damper %s  envs %d  k in [%.1f, %.1f]  %d substeps per env step  shift %.3f m  IMU sites %s on bodies %s"
          % (args.scene, args.tendon_damper, n, ks[0], ks[-1], args.substeps, args.shift, imu, [int(body[s]) for s in imu]))
    print("# step flagged max|virtual - sensordata|  then per IMU site and per placement (%s): median |accel| m/s^2, median |gyro| rad/s" % " ".join(x for x, _ in shifts))
    for t in range(args.steps):
        if args.substeps > 1:
            b.step(args.substeps - 1, sens=sens, flags=flags)
        st = b.get_state()
        b.step(1, sens=sens, flags=flags)
        out = b.point_motion(pb, pp, pq, qpos=st["qpos"], qvel=st["qvel"], qacc=b.get_state()["qacc_warmstart"], outputs=("gyro", "accel"))
        gy, ac, sd = out["gyro"].cpu().numpy(), out["accel"].cpu().numpy(), sens.cpu().numpy()
        ok = (flags == 0).cpu().numpy()
        dev = 0.0
        cells = []
        for i, s in enumerate(imu):
            for kind, arr in (("accel", ac), ("gyro", gy)):
                if kind in chan[s] and ok.any():
                    dev = max(dev, float(np.abs(arr[ok, i * P] - sd[ok, chan[s][kind]:chan[s][kind] + 3]).max()))
            cells.append("site %d:" % s + " ".join("%s %.4f %.4f" % (name, np.median(np.linalg.norm(ac[ok, i * P + j], axis=1)) if ok.any() else np.nan,
                                                                  np.median(np.linalg.norm(gy[ok, i * P + j], axis=1)) if ok.any() else np.nan)
                                                     for j, (name, _) in enumerate(shifts)))
        print("%3d %2d %.3e  %s" % (t, int((~ok).sum()), dev, "  ".join(cells)))


if __name__ == "__main__":
    main()
