"""Timings (HIP events) of sg_get_forces on the GPU: time per call at 64 and at all listed envs of a 4096-env batch ten env steps into a
squeeze, beside one sg_step (7 substeps, one env step) of the same batch measured in the same run, with the number of chunks the env
list is processed in at the work-space cap in force (--workspace-mib; the default is the library's 256 MiB).  The timed calls are the C
entry point on buffers allocated once; the step is timed from the state the forces were timed at, seated again before every timed
step.  Median of --windows windows of --reps calls.  No threshold: the numbers are what DESIGN.md 8.9 quotes.

usage: python scripts/forces_bench.py [--envs 4096] [--scenes softbox,softball,fourfinger_softball] [--listed 64,4096] [--windows 2] [--reps 1]
                                      [--workspace-mib 256] [--out profiles/r23_forces_readout_bench.json]"""
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
SCENES = {"softbox": (None, list(range(11, 64)), [0], 2), "softball": (None, list(range(11, 64)), [0], 2),
          "fourfinger_softball": ("implicit", list(range(65, 283)), [0], 4)}


def env_bytes(rows, cap, nv):
    """one env's share of the call's work space (csrc/sg_forces.h: sgf_env_doubles, sgf_env_ints)"""
    return 8 * (2 * rows * nv + 8 * rows + nv + 13 * cap + (3 * rows + 3 * cap + 5) // 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--scenes", default="softbox,softball,fourfinger_softball")
    ap.add_argument("--listed", default="64,4096")
    ap.add_argument("--windows", type=int, default=2)
    ap.add_argument("--reps", type=int, default=1)
    ap.add_argument("--workspace-mib", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import softgrip_amd as sg
    from softgrip_amd import native
    from softgrip_amd.native import _ptr
    res = {"envs": args.envs, "windows": args.windows, "reps": args.reps, "workspace_mib": args.workspace_mib, "device": torch.cuda.get_device_name(0), "scenes": {}}
    for scene in args.scenes.split(","):
        damper, jids, tids, nu = SCENES[scene]
        m = sg.load_model(os.path.join(ROOT, "models", scene + ".sgmodel"), damper)
        nm = native.NativeModel(m)
        b = native.NativeBatch(nm, args.envs, 0)
        b.set_stiffness(np.random.RandomState(0).uniform(300, 1400, args.envs), jids, tids)
        flags = torch.zeros(args.envs, dtype=torch.int32, device=b.device)
        b.reset(1, flags=flags)
        b.set_ctrl_broadcast(np.full(nu, -0.2))
        for _ in range(10):
            b.step(7, flags=flags)
        b.set_forces_workspace(args.workspace_mib << 20)
        rows, cap = b.max_rows(), int(m.nconmax) if 0 < int(m.nconmax) < 512 else 512
        per_env = env_bytes(rows, cap, nm.nv)
        state = b.get_state()
        seat = lambda: b.set_state(qpos=state["qpos"], qvel=state["qvel"], act=state["act"], qacc_warmstart=state["qacc_warmstart"], ctrl=state["ctrl"])  # noqa: E731
        out = {"model": dict(nv=nm.nv, max_rows=rows, env_bytes=per_env)}
        L, s = b.L, b._stream()
        for listed in (int(x) for x in args.listed.split(",")):
            listed = min(listed, args.envs)
            ids = None if listed == args.envs else np.arange(listed, dtype=np.int32)
            arr = None if ids is None else ids.ctypes.data_as(C.POINTER(C.c_int32))
            o = b.forces(env_ids=ids, max_contacts=8)      # the outputs, allocated ONCE: the timed calls are the C entry point on these buffers
            order = ("nefc", "iters", "efc_type", "efc_id", "efc_force", "ncon", "contact_force", "qfrc_constraint", "qacc")
            ptrs = [_ptr(o[name]) for name in order]
            call = lambda: L.sg_get_forces(b.ptr, arr, listed, rows, 8, *ptrs, s)  # noqa: E731
            assert not call(), L.sg_last_error()
            torch.cuda.synchronize()
            nefc, iters = o["nefc"].cpu().numpy(), o["iters"].cpu().numpy()
            t = windows(torch, call, args.reps, args.windows)
            t.update(chunks=-(-listed // max((args.workspace_mib << 20) // per_env, 1)), nefc_mean=float(nefc.mean()), nefc_max=int(nefc.max()),
                     iters_mean=float(iters.mean()), ncon_mean=float(o["ncon"].float().mean()))
            out["sg_get_forces_%d" % listed] = t
        # the yardstick: one env step of the same batch FROM THE SAME STATE -- seated again before every timed step, outside the timing
        w = []
        for _ in range(args.windows * args.reps):
            seat()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            b.step(7, flags=flags)
            e1.record()
            e1.synchronize()
            w.append(e0.elapsed_time(e1))
        out["sg_step_7_substeps"] = {"windows_ms": w, "median_ms": float(np.median(w)), "min_ms": min(w), "max_ms": max(w)}
        seat()
        for name in [k for k in out if k.startswith("sg_get_forces")]:
            out[name]["ratio_to_sg_step"] = out[name]["median_ms"] / out["sg_step_7_substeps"]["median_ms"]
        out["flagged_envs"] = int((flags != 0).sum())
        res["scenes"][scene] = out
        print(scene, {k: (round(v["median_ms"], 3), v.get("chunks")) for k, v in out.items() if isinstance(v, dict) and "median_ms" in v}, flush=True)
        save(res, args.out)
        del b
    if not args.out:
        print(json.dumps(res, indent=1))


def save(res, path):
    """the results so far: written after every scene, so that a run cut short keeps what it measured"""
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
