"""Contact read-out timings (HIP events) on the GPU: sg_get_contacts for all envs of a 4096-env batch against ONE sg_step call (7 substeps:
seven collision passes plus seven solves) of the same batch in the same process, at the reset state and at env step 100 of the squeeze.

  scenes: softbox, softcylinder (rows pipeline), fourfinger_softball_fix, freeball_fix (tree pipeline)

Both are timed as a window of `reps` back-to-back calls between two events after a warm-up call, alternating the two windows `rounds`
times; the figure is the median window / reps.  The step windows advance the state, so the batch is put back on the sampled state
(sg_set_state) before every window and both always see the same state.  The read-out must take less time than the step.

usage: python scripts/contacts_bench.py [--envs 4096] [--reps 10] [--rounds 5] [--out profiles/r06_contacts_bench.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCENES = {"softbox": (None, list(range(11, 64)), 2), "softcylinder": ("implicit", list(range(11, 64)), 2),
          "fourfinger_softball_fix": ("implicit", list(range(65, 283)), 4), "freeball_fix": ("implicit", list(range(9, 227)), 2)}
MAXC = 256


def window(torch, fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--scenes", nargs="*", default=list(SCENES))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import softgrip_amd as sg
    from softgrip_amd import native
    from softgrip_amd.create_dataset import episode_schedule
    if not torch.cuda.is_available():
        sys.exit("contacts_bench.py needs a GPU: there is nothing to time without one")
    res = {"device": torch.cuda.get_device_name(0), "envs": args.envs, "reps": args.reps, "rounds": args.rounds, "max_contacts": MAXC,
           "method": "HIP events around `reps` back-to-back calls, median over `rounds` alternating windows, ms per call", "cases": []}
    sched = episode_schedule()
    for scene in args.scenes:
        damper, jids, nu = SCENES[scene]
        m = sg.load_model(os.path.join(ROOT, "models", scene + ".sgmodel"), damper)
        nm = native.NativeModel(m)
        b = native.NativeBatch(nm, args.envs, 0)
        b.set_stiffness(np.random.RandomState(0).uniform(300, 1400, args.envs), jids, [0])
        flags = torch.zeros(args.envs, dtype=torch.int32, device=b.device)
        sens = torch.zeros(args.envs, nm.nsensordata, dtype=torch.float64, device=b.device)
        b.reset(1, sens=sens, flags=flags)
        kw = dict(device=b.device)
        out = dict(ncon=torch.zeros(args.envs, dtype=torch.int32, **kw), geom=torch.zeros(args.envs, MAXC, 2, dtype=torch.int32, **kw),
                   dist=torch.zeros(args.envs, MAXC, dtype=torch.float64, **kw), pos=torch.zeros(args.envs, MAXC, 3, dtype=torch.float64, **kw),
                   frame=torch.zeros(args.envs, MAXC, 9, dtype=torch.float64, **kw))

        def measure(label):
            st = b.get_state()

            def restore():
                b.set_state(qpos=st["qpos"], qvel=st["qvel"], act=st["act"], qacc_warmstart=st["qacc_warmstart"], ctrl=st["ctrl"])
            b.contacts_into(out)                         # warm-up of both (first launches load the code objects)
            b.step(7, sens=sens, flags=flags)
            tc, ts = [], []
            for _ in range(args.rounds):
                restore()
                torch.cuda.synchronize()
                tc.append(window(torch, lambda: b.contacts_into(out), args.reps))
                ts.append(window(torch, lambda: b.step(7, sens=sens, flags=flags), args.reps))
            restore()
            b.contacts_into(out)
            ncon = out["ncon"].cpu().numpy()
            case = {"scene": scene, "state": label, "ngeom": nm.ngeom, "nbody": nm.nbody, "candidate_pairs": nm.ncollision_pairs,
                    "ncon_mean": float(ncon[ncon >= 0].mean()) if (ncon >= 0).any() else None, "ncon_max": int(ncon.max()),
                    "envs_not_finite": int((ncon < 0).sum()),
                    "get_contacts_ms": float(np.median(tc)), "get_contacts_ms_windows": [float(x) for x in tc],
                    "step_ms": float(np.median(ts)), "step_ms_windows": [float(x) for x in ts]}
            case["read_out_over_step"] = case["get_contacts_ms"] / case["step_ms"]
            case["faster_than_one_step"] = case["get_contacts_ms"] < case["step_ms"]
            res["cases"].append(case)
            print(json.dumps(case), flush=True)

        measure("reset")
        for t in range(100):
            if sched[t] is not None:
                b.set_ctrl_broadcast(np.full(nu, sched[t]))
            b.step(7, sens=sens, flags=flags)
        measure("env step 100")
        del b
    res["all_faster_than_one_step"] = all(c["faster_than_one_step"] for c in res["cases"])
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print("all faster than one sg_step: %s" % res["all_faster_than_one_step"])


if __name__ == "__main__":
    main()
