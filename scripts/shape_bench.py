"""Timings (HIP events) of sg_get_skin_vertices, sg_get_shape (the shape and six directions) and sg_get_subtree on the GPU at 1, 64 and
all listed envs of a 4096-env batch ten env steps into a squeeze, with sg_get_velocities on the same lists beside them as the
yardstick (the same body walk, three per-body arrays out).  The timed calls are the C entry points on buffers allocated once.  Median
of --windows windows of --reps calls.  No threshold: the numbers are what DESIGN.md 8.10 quotes.

usage: python scripts/shape_bench.py [--envs 4096] [--scenes softbox,softball] [--listed 1,64,4096] [--windows 5] [--reps 10]
                                     [--out profiles/r24_shape_readout_bench.json]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from forces_bench import save  # noqa: E402
from smooth_bench import windows  # noqa: E402

# scene -> (tendon damper, joints / tendons that take the per-env stiffness, actuators)
SCENES = {"softbox": (None, list(range(11, 64)), [0], 2), "softball": (None, list(range(11, 64)), [0], 2)}
DIRS = np.array([[1.0, 0, 0], [0, 1, 0], [0, 0, 1], [0.3, -2.0, 0.7], [1.0, 0, 0], [0, 0.5, 0.5]])
DIR_BODY = np.array([-1, -1, -1, -1, 3, 3], np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--scenes", default="softbox,softball")
    ap.add_argument("--listed", default="1,64,4096")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import softgrip_amd as sg
    from softgrip_amd import native
    from softgrip_amd.native import _ptr
    res = {"envs": args.envs, "windows": args.windows, "reps": args.reps, "device": torch.cuda.get_device_name(0), "n_dirs": len(DIRS), "scenes": {}}
    for scene in args.scenes.split(","):
        damper, jids, tids, nu = SCENES[scene]
        m = sg.load_model(os.path.join(ROOT, "models", scene + ".sgmodel"), damper)
        nm = native.NativeModel(m)
        nm.set_skin(m.composite_skin())
        b = native.NativeBatch(nm, args.envs, 0)
        b.set_stiffness(np.random.RandomState(0).uniform(300, 1400, args.envs), jids, tids)
        flags = torch.zeros(args.envs, dtype=torch.int32, device=b.device)
        b.reset(1, flags=flags)
        b.set_ctrl_broadcast(np.full(nu, -0.2))
        for _ in range(10):
            b.step(7, flags=flags)
        root = nm.skin_root()
        out = {"model": dict(nbody=nm.nbody, nvert=b.nvert(), nface=int(len(nm.skin()["face"])), object_body=root, lds_bytes=8 * (22 * nm.nbody + 6 * b.nvert()))}
        L, s = b.L, b._stream()
        dp, bp = DIRS.ctypes.data_as(C.c_void_p), DIR_BODY.ctypes.data_as(C.POINTER(C.c_int32))
        for listed in (int(x) for x in args.listed.split(",")):
            listed = min(listed, args.envs)
            ids = None if listed == args.envs else np.arange(listed, dtype=np.int32)
            arr = None if ids is None else ids.ctypes.data_as(C.POINTER(C.c_int32))
            v, sh, st, ve = b.skin_vertices(root, env_ids=ids), b.shape(DIRS, DIR_BODY, env_ids=ids), b.subtree(env_ids=ids), b.velocities(env_ids=ids)
            calls = {
                "sg_get_skin_vertices": lambda: L.sg_get_skin_vertices(b.ptr, arr, listed, root, _ptr(v["pos"]), _ptr(v["vel"]), _ptr(v["local"]), s),
                "sg_get_shape": lambda: L.sg_get_shape(b.ptr, arr, listed, len(DIRS), dp, bp, _ptr(sh["shape"]), _ptr(sh["lo"]), _ptr(sh["hi"]), _ptr(sh["lo_vert"]),
                                                       _ptr(sh["hi_vert"]), s),
                "sg_get_shape_no_dirs": lambda: L.sg_get_shape(b.ptr, arr, listed, 0, None, None, _ptr(sh["shape"]), None, None, None, None, s),
                "sg_get_subtree": lambda: L.sg_get_subtree(b.ptr, arr, listed, _ptr(st["com"]), _ptr(st["linvel"]), _ptr(st["angmom"]), s),
                "sg_get_velocities": lambda: L.sg_get_velocities(b.ptr, arr, listed, _ptr(ve["ang"]), _ptr(ve["lin"]), _ptr(ve["com_lin"]), s),
            }
            for name, call in calls.items():
                assert not call(), L.sg_last_error()
                torch.cuda.synchronize()
                out["%s_%d" % (name, listed)] = windows(torch, call, args.reps, args.windows)
            yard = out["sg_get_velocities_%d" % listed]["median_ms"]
            for name in calls:
                out["%s_%d" % (name, listed)]["ratio_to_sg_get_velocities"] = out["%s_%d" % (name, listed)]["median_ms"] / yard
        out["flagged_envs"] = int((flags != 0).sum())
        res["scenes"][scene] = out
        print(scene, {k: round(x["median_ms"], 4) for k, x in out.items() if isinstance(x, dict) and "median_ms" in x}, flush=True)
        save(res, args.out)
        del b
    if not args.out:
        print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
