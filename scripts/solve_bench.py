"""Timings (HIP events) of the read-outs that start with the inverse of the mass matrix on the GPU: sg_solve_mass at n_rhs = 1 and 16,
sg_forward_smooth, sg_get_point_inertia at the model's sensor sites, against sg_get_mass_matrix and sg_inverse_dynamics of the same batch
in the same run -- all read the same state and walk the same tree.  4096 envs five env steps into a squeeze; median of 5 windows of 10
calls.  Which stage dominates is read from three more calls: sg_get_joint_forces asking for bias alone (the forward and backward walks),
sg_solve_mass asking for pivot alone (the walks, the packed M and its factor, no solve) and the full call.  No threshold: the numbers
are what DESIGN.md 8.8 quotes.

usage: python scripts/solve_bench.py [--envs 4096] [--scenes softbox,fourfinger_softball_fix] [--windows 5] [--reps 10] [--out FILE.json]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from smooth_bench import windows  # noqa: E402

# scene -> (tendon damper, joints / tendons that take the per-env stiffness, actuators)
SCENES = {"softbox": (None, list(range(11, 64)), [0], 2), "fourfinger_softball_fix": ("implicit", list(range(65, 283)), [0], 4),
          "freeball_fix": ("implicit", list(range(9, 227)), [0], 2)}
YARDSTICKS = ("sg_get_mass_matrix", "sg_inverse_dynamics")


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
    from softgrip_amd.mjcf import SENS_ACCELEROMETER, SENS_GYRO
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
        n, nb, nv = args.envs, nm.nbody, nm.nv
        sbody, spos, _ = nm.sites()
        imu = sorted({int(m.sensor_objid[s]) for s in range(len(m.sensor_type)) if int(m.sensor_type[s]) in (SENS_ACCELEROMETER, SENS_GYRO)})
        sbody, spos = np.ascontiguousarray(sbody[imu]), np.ascontiguousarray(spos[imu])
        P = len(sbody)
        M = torch.empty(n, nv, nv, **kw)
        bias, inv, qa, qf = (torch.empty(n, nv, **kw) for _ in range(4))
        qacc, y1, y16 = torch.randn(n, nv, **kw), torch.randn(n, 1, nv, **kw), torch.randn(n, 16, nv, **kw)
        x1, x16 = torch.empty_like(y1), torch.empty_like(y16)
        W, pivot = torch.empty(n, P, 6, 6, **kw), torch.empty(n, **kw)
        L, s = b.L, b._stream()
        pb, pp = sbody.ctypes.data_as(C.POINTER(C.c_int32)), spos.ctypes.data_as(C.c_void_p)
        calls = {
            "sg_get_mass_matrix": lambda: L.sg_get_mass_matrix(b.ptr, None, n, _ptr(M), s),
            "sg_inverse_dynamics": lambda: L.sg_inverse_dynamics(b.ptr, None, n, _ptr(qacc), _ptr(inv), s),
            "walks_alone": lambda: L.sg_get_joint_forces(b.ptr, None, n, _ptr(bias), None, None, s),
            "factor_alone": lambda: L.sg_solve_mass(b.ptr, None, n, 1, _ptr(y1), None, _ptr(pivot), s),
            "sg_solve_mass_1": lambda: L.sg_solve_mass(b.ptr, None, n, 1, _ptr(y1), _ptr(x1), _ptr(pivot), s),
            "sg_solve_mass_16": lambda: L.sg_solve_mass(b.ptr, None, n, 16, _ptr(y16), _ptr(x16), _ptr(pivot), s),
            "sg_forward_smooth": lambda: L.sg_forward_smooth(b.ptr, None, n, None, _ptr(qa), _ptr(qf), _ptr(pivot), s),
            "sg_get_point_inertia": lambda: L.sg_get_point_inertia(b.ptr, None, n, P, pb, pp, _ptr(W), _ptr(pivot), s),
        }
        for name, fn in calls.items():
            assert not fn(), (name, L.sg_last_error())
        torch.cuda.synchronize()
        out = {name: windows(torch, fn, args.reps, args.windows) for name, fn in calls.items()}
        for base in YARDSTICKS:
            for name in calls:
                out[name]["ratio_to_" + base[3:]] = out[name]["median_ms"] / out[base]["median_ms"]
        walks, factor = out["walks_alone"]["median_ms"], out["factor_alone"]["median_ms"]
        out["stages_ms"] = {"walks": walks, "packed_M_and_factor": factor - walks,
                            **{name + "_rhs_solve_store": out[name]["median_ms"] - factor
                               for name in ("sg_solve_mass_1", "sg_solve_mass_16", "sg_forward_smooth", "sg_get_point_inertia")}}
        out["model"] = dict(nbody=nb, nv=nv, sensor_sites=P, pivot_min=float(pivot.min()), flagged_envs=int((flags != 0).sum()))
        out["bytes_moved"] = {"sg_get_mass_matrix": n * nv * nv * 8, "sg_solve_mass_1": 2 * n * nv * 8, "sg_solve_mass_16": 32 * n * nv * 8,
                              "sg_forward_smooth": 2 * n * nv * 8, "sg_get_point_inertia": n * P * 36 * 8}
        res["scenes"][scene] = out
        print(scene, {k: round(v["median_ms"], 4) for k, v in out.items() if "median_ms" in v}, {k: round(v, 4) for k, v in out["stages_ms"].items()})
        del M
    text = json.dumps(res, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    else:
        print(text)


if __name__ == "__main__":
    main()
