"""Timings (HIP events) of the point read-outs on the GPU: sg_get_point_motion at the model's sites (all six outputs, the virtual-IMU
call), sg_get_jacobians at the model's sites and at one point per body, against sg_get_poses (xpos + xquat) and sg_get_velocities of
the same batch in the same run -- all read the same state and walk the same tree.  4096 envs five env steps into a squeeze; median of 5
windows of 10 calls.  The Jacobian calls write 2 x n_pts x 3 x nv x 8 bytes per env: beside their time stand the bytes written, the
write rate achieved, and a device-to-device copy of as many bytes in the same run (a copy reads and writes them: twice the traffic).
No threshold: the numbers are what DESIGN.md 8.7 quotes.

usage: python scripts/point_bench.py [--envs 4096] [--scenes softbox,fourfinger_softball_fix] [--windows 5] [--reps 10] [--out FILE.json]"""
import argparse
import ctypes as C
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# scene -> (tendon damper, joints that take the per-env stiffness, tendons that take it, number of actuators)
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
    hdr = open(os.path.join(ROOT, "soft-grip_amd", "csrc", "sg_point.h")).read()      # the record sizes the kernel's LDS block is made of
    rec, dof = (int(re.search(r"#define %s (\d+)" % name, hdr).group(1)) for name in ("SGP_REC", "SGP_DOF"))
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
        xpos, xquat = torch.empty(n, nb, 3, **kw), torch.empty(n, nb, 4, **kw)
        ang, lin, com = (torch.empty(n, nb, 3, **kw) for _ in range(3))
        qacc = b.get_state()["qacc_warmstart"]
        sb, sp, sq = nm.sites()
        bb, bp = np.arange(nb, dtype=np.int32), np.ascontiguousarray(m.body_ipos, dtype=np.float64).reshape(nb, 3)
        ns = len(sb)
        mot = [torch.empty(n, ns, w, **kw) for w in (3, 9, 6, 6, 3, 3)]
        ip, vp = (lambda x: x.ctypes.data_as(C.POINTER(C.c_int32))), (lambda x: x.ctypes.data_as(C.c_void_p))
        L, s = b.L, b._stream()
        calls = {
            "sg_get_poses": lambda: L.sg_get_poses(b.ptr, None, n, _ptr(xpos), _ptr(xquat), None, None, s),
            "sg_get_velocities": lambda: L.sg_get_velocities(b.ptr, None, n, _ptr(ang), _ptr(lin), _ptr(com), s),
            "motion_at_sites": lambda: L.sg_get_point_motion(b.ptr, None, n, ns, ip(sb), vp(sp), vp(sq), None, None, _ptr(qacc), *[_ptr(x) for x in mot], s),
            "gyro_accel_at_sites": lambda: L.sg_get_point_motion(b.ptr, None, n, ns, ip(sb), vp(sp), vp(sq), None, None, _ptr(qacc), None, None, None, None,
                                                                 _ptr(mot[4]), _ptr(mot[5]), s),
        }
        jac = {}
        for name, (body, pos) in (("jacobians_at_sites", (sb, sp)), ("jacobians_per_body", (bb, bp))):
            jp, jr = torch.empty(n, len(body), 3, nv, **kw), torch.empty(n, len(body), 3, nv, **kw)
            jac[name] = (jp, jr)
            calls[name] = (lambda body=body, pos=pos, jp=jp, jr=jr: L.sg_get_jacobians(b.ptr, None, n, len(body), ip(body), vp(pos), None, _ptr(jp), _ptr(jr), s))
        for name, fn in calls.items():
            assert not fn(), (name, L.sg_last_error())
        out = {name: windows(torch, fn, args.reps, args.windows) for name, fn in calls.items()}
        for base in ("sg_get_poses", "sg_get_velocities"):
            for name in calls:
                out[name]["ratio_to_" + base[7:]] = out[name]["median_ms"] / out[base]["median_ms"]
        out["motion_at_sites"]["bytes_written"] = n * ns * 30 * 8
        for name, (jp, jr) in jac.items():
            nbytes = 2 * jp.numel() * 8
            dst = torch.empty_like(jp)
            cp = windows(torch, lambda: (dst.copy_(jp), dst.copy_(jr)), args.reps, args.windows)
            del dst
            out[name].update(n_pts=jp.shape[1], bytes_written=nbytes, achieved_write_bytes_per_s=nbytes / (out[name]["median_ms"] * 1e-3),
                             copy_of_as_many_bytes_ms=cp["median_ms"], copy_bandwidth_bytes_per_s=2 * nbytes / (cp["median_ms"] * 1e-3),
                             write_alone_at_copy_bandwidth_ms=nbytes / (2 * nbytes / (cp["median_ms"] * 1e-3)) * 1e3)
        out["model"] = dict(nbody=nb, nv=nv, nsite=ns, lds_bytes=8 * (rec * nb + dof * nv) + 4 * nv, flagged_envs=int((flags != 0).sum()))
        res["scenes"][scene] = out
        print(scene, {k: round(v["median_ms"], 4) for k, v in out.items() if "median_ms" in v},
              {k: "%.2f TB/s" % (v["achieved_write_bytes_per_s"] / 1e12) for k, v in out.items() if "achieved_write_bytes_per_s" in v})
        del jac, calls
    text = json.dumps(res, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    else:
        print(text)


if __name__ == "__main__":
    main()
