"""Timings (HIP events) of the velocity / tendon / energy read-outs on the GPU: sg_get_velocities, sg_get_tendons, sg_get_energy, each alone
and the three in a row, against sg_get_poses (xpos + xquat) of the same batch in the same run -- both read the same state and walk the
same tree.  4096 envs a few env steps into a squeeze; median of 5 windows of 10 calls.  No threshold: the numbers are what DESIGN.md 8.5
quotes.

usage: python scripts/dyn_bench.py [--envs 4096] [--scenes softbox,fourfinger_softball_fix] [--windows 5] [--reps 10] [--out profiles/r18_dyn_readout_bench.json]"""
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
        n, nb, nt = args.envs, nm.nbody, nm.ntendon
        xpos, xquat = torch.empty(n, nb, 3, **kw), torch.empty(n, nb, 4, **kw)
        ang, lin, com = (torch.empty(n, nb, 3, **kw) for _ in range(3))
        length, vel, en = torch.empty(n, nt, **kw), torch.empty(n, nt, **kw), torch.empty(n, 4, **kw)
        L, s = b.L, b._stream()
        calls = {
            "sg_get_poses": lambda: L.sg_get_poses(b.ptr, None, n, _ptr(xpos), _ptr(xquat), None, None, s),
            "sg_get_velocities": lambda: L.sg_get_velocities(b.ptr, None, n, _ptr(ang), _ptr(lin), _ptr(com), s),
            "sg_get_tendons": lambda: L.sg_get_tendons(b.ptr, None, n, _ptr(length), _ptr(vel), s),
            "sg_get_energy": lambda: L.sg_get_energy(b.ptr, None, n, _ptr(en), s),
        }
        calls["all_three"] = lambda: (calls["sg_get_velocities"](), calls["sg_get_tendons"](), calls["sg_get_energy"]())
        for name, fn in calls.items():
            rc = fn()
            assert not (rc if isinstance(rc, int) else any(rc)), (name, L.sg_last_error())
        out = {name: windows(torch, fn, args.reps, args.windows) for name, fn in calls.items()}
        base = out["sg_get_poses"]["median_ms"]
        for name in out:
            out[name]["ratio_to_poses"] = out[name]["median_ms"] / base
        out["model"] = dict(nbody=nb, nv=nm.nv, ntendon=nt, lds_bytes=13 * 8 * nb, flagged_envs=int((flags != 0).sum()))
        out["bytes_written"] = {"sg_get_poses": n * nb * 7 * 8, "sg_get_velocities": n * nb * 9 * 8, "sg_get_tendons": n * nt * 16, "sg_get_energy": n * 32}
        res["scenes"][scene] = out
        print(scene, {k: round(v["median_ms"], 4) for k, v in out.items() if "median_ms" in v})
    text = json.dumps(res, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    else:
        print(text)


if __name__ == "__main__":
    main()
