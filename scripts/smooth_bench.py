"""Timings (HIP events) of the mass-matrix / joint-force / inverse-dynamics read-outs on the GPU: sg_get_mass_matrix (with its output
write, and the same walk without it: sg_get_joint_forces asking for bias alone runs the forward and backward walks and skips M),
sg_get_joint_forces, sg_inverse_dynamics, against sg_get_poses (xpos + xquat) and sg_get_velocities of the same batch in the same run --
all read the same state and walk the same tree.  4096 envs five env steps into a squeeze; median of 5 windows of 10 calls.  The M call
writes nv^2 8 bytes per env: its time is also given as the share of it that the write alone would take at the HBM bandwidth measured
in the same run (a device-to-device copy of the same number of bytes).  No threshold: the numbers are what DESIGN.md 8.6 quotes.

usage: python scripts/smooth_bench.py [--envs 4096] [--scenes softbox,fourfinger_softball_fix] [--windows 5] [--reps 10] [--out FILE.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# scene -> (tendon damper, joints / tendons that take the per-env stiffness, actuators)
SCENES = {"softbox": (None, list(range(11, 64)), [0], 2), "fourfinger_softball_fix": ("implicit", list(range(65, 283)), [0], 4)}


def timed(torch, fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def windows(torch, fn, reps, n):
    w = [timed(torch, fn, reps) for _ in range(n)]
    return {"windows_ms": w, "median_ms": float(np.median(w)), "min_ms": min(w), "max_ms": max(w)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--scenes", default="softbox,fourfinger_softball_fix")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import softgrip_amd as sg
    from softgrip_amd import native
    from softgrip_amd.native import _ptr
    res = {"envs": args.envs, "windows": args.windows, "reps": args.reps, "device": torch.cuda.get_device_name(0), "scenes": {}}
    for scene in args.scenes.split(","):
        damper, jids, tids, nu = SCENES[scene]
        m = sg.load_model(os.path.join(ROOT, "models", scene + ".sgmodel"), damper)
        nm = native.NativeModel(m)
        b = native.NativeBatch(nm, args.envs, 0)
        b.set_stiffness(np.random.RandomState(0).uniform(300, 1400, args.envs), jids, tids)
        flags = torch.zeros(args.envs, dtype=torch.int32, device=b.device)
        b.reset(1, flags=flags)
        b.set_ctrl_broadcast(np.full(nu, -0.2))
        for _ in range(5):
            b.step(7, flags=flags)
        kw = dict(dtype=torch.float64, device=b.device)
        n, nb, nv, nt = args.envs, nm.nbody, nm.nv, nm.ntendon
        xpos, xquat = torch.empty(n, nb, 3, **kw), torch.empty(n, nb, 4, **kw)
        ang, lin, com = (torch.empty(n, nb, 3, **kw) for _ in range(3))
        M, copy = torch.empty(n, nv, nv, **kw), torch.empty(n, nv, nv, **kw)
        bias, passive, actuator, inv = (torch.empty(n, nv, **kw) for _ in range(4))
        qacc = torch.randn(n, nv, **kw)
        L, s = b.L, b._stream()
        calls = {
            "sg_get_poses": lambda: L.sg_get_poses(b.ptr, None, n, _ptr(xpos), _ptr(xquat), None, None, s),
            "sg_get_velocities": lambda: L.sg_get_velocities(b.ptr, None, n, _ptr(ang), _ptr(lin), _ptr(com), s),
            "sg_get_mass_matrix": lambda: L.sg_get_mass_matrix(b.ptr, None, n, _ptr(M), s),
            "walks_without_M_write": lambda: L.sg_get_joint_forces(b.ptr, None, n, _ptr(bias), None, None, s),
            "sg_get_joint_forces": lambda: L.sg_get_joint_forces(b.ptr, None, n, _ptr(bias), _ptr(passive), _ptr(actuator), s),
            "sg_inverse_dynamics": lambda: L.sg_inverse_dynamics(b.ptr, None, n, _ptr(qacc), _ptr(inv), s),
        }
        for name, fn in calls.items():
            assert not fn(), (name, L.sg_last_error())
        out = {name: windows(torch, fn, args.reps, args.windows) for name, fn in calls.items()}
        out["copy_of_M_bytes"] = windows(torch, lambda: copy.copy_(M), args.reps, args.windows)      # (reads and writes the bytes: 2 x the traffic)
        for base in ("sg_get_poses", "sg_get_velocities"):
            for name in calls:
                out[name]["ratio_to_" + base[7:]] = out[name]["median_ms"] / out[base]["median_ms"]
        mbytes = n * nv * nv * 8
        bw = 2 * mbytes / (out["copy_of_M_bytes"]["median_ms"] * 1e-3)
        out["M_write"] = dict(bytes=mbytes, copy_bandwidth_bytes_per_s=bw, write_alone_ms=mbytes / bw * 1e3,
                              share_of_M_call=mbytes / bw * 1e3 / out["sg_get_mass_matrix"]["median_ms"],
                              achieved_write_bytes_per_s=mbytes / (out["sg_get_mass_matrix"]["median_ms"] * 1e-3))
        out["model"] = dict(nbody=nb, nv=nv, ntendon=nt, lds_bytes=8 * (29 * nb + 7 * nv + 2 * nt), flagged_envs=int((flags != 0).sum()))
        out["bytes_written"] = {"sg_get_poses": n * nb * 7 * 8, "sg_get_velocities": n * nb * 9 * 8, "sg_get_mass_matrix": mbytes,
                                "sg_get_joint_forces": n * nv * 24, "sg_inverse_dynamics": n * nv * 8}
        res["scenes"][scene] = out
        print(scene, {k: round(v["median_ms"], 4) for k, v in out.items() if "median_ms" in v}, "M write share %.2f" % out["M_write"]["share_of_M_call"])
        del M, copy
    text = json.dumps(res, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    else:
        print(text)


if __name__ == "__main__":
    main()
