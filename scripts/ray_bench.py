"""Ray query timings (HIP events) on the GPU: sg_ray against ONE sg_step call (7 substeps) of the same batch in the same process, at env
step 100 of the squeeze, softbox, 4096 envs.

  (a) ManEnv.tactile_depth's rays at 8 x 8 (nboxes x 64 body-frame rays per env, own body excluded, elements + centre), all envs
  (b) one world-frame ray per env (a rangefinder), all envs
  (c) n_rays swept over 1, 4, 16, 64, 256, 1024 under both forced layouts (SG_RAY_LAYOUT): the crossover of the automatic choice
  (d) 16 envs x 320 x 240 camera rays through sg_ray next to sg_render depth-only on the same camera

The method of scripts/contacts_bench.py: each figure is a window of `reps` back-to-back calls between two events after a warm-up call,
alternating with a window of sg_step on the same batch `rounds` times; the figure is the median window / reps.  The step windows
advance the state, so the batch is put back on the sampled state (sg_set_state) before every window.

--skin: the same method for sg_ray with SG_RAY_SKIN, on softball (implicit damper) at env step 20 of the squeeze:
  (a) the 8 x 8 tactile map against the skin and against the capsules (the plain call), automatic choice and both forced layouts
  (b) n_rays swept over 1 ... 1024 under both forced layouts with the flag: the crossing point of the skin path
  (c) the plain call's (a) figures once more from another build of the library, measured in the same session: run the script with
      --skin --plain-only under SOFTGRIP_LIB=<that build> first and hand its --out to this run as --parent-json (of a full --skin result
      only the plain call's cases are copied)
  --stages: nothing is timed; the tactile map is cast `reps` times against the skin and `reps` times against the capsules, for a run
      under `rocprofv3 --kernel-trace --stats -- python scripts/ray_bench.py --skin --stages`: the per-kernel split of the call

Every timed query's outputs (dist, geom ids and, written by that call alone, the normals) are hashed (SHA-256, one more call on the
sampled state) into its case; with --parent-json
FILE, the result of the same command under SOFTGRIP_LIB=<another build>, the digests are compared case by case: SAME or DIFFERENT.

usage: python scripts/ray_bench.py [--envs 4096] [--reps 10] [--rounds 5] [--out profiles/r08_ray_bench.json]
       python scripts/ray_bench.py --skin [--plain-only] [--parent-json FILE] [--out profiles/r10_ray_skin_bench.json]"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def window(torch, fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def digest(torch, fn):
    """SHA-256 of what a timed query wrote (its `outputs`: device tensors), None for a call without any"""
    outs = getattr(fn, "outputs", ())
    if not outs:
        return None
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in outs:
        h.update(t.cpu().numpy().tobytes())
    return h.hexdigest()


def bits_against(res, parent):
    """per case of this run that the other build's run has too: SAME or DIFFERENT output digests; printed, and kept under 'bits_vs_parent'"""
    theirs = {(c["case"], c["layout"]): c.get("sha256") for c in parent["cases"]}
    out = []
    for c in res["cases"]:
        key = (c["case"], c["layout"])
        if c.get("sha256") and theirs.get(key):
            out.append({"case": key[0], "layout": key[1], "bits": "SAME" if c["sha256"] == theirs[key] else "DIFFERENT"})
            print("%-9s %s [%s]" % (out[-1]["bits"], key[0], key[1]), flush=True)
    res["bits_vs_parent"] = {"library": parent.get("library"), "cases": out, "different": sum(x["bits"] == "DIFFERENT" for x in out)}
    print("bits against the other build: %d cases, %d DIFFERENT" % (len(out), res["bits_vs_parent"]["different"]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skin", action="store_true", help="time SG_RAY_SKIN on softball at env step 20 instead")
    ap.add_argument("--plain-only", action="store_true", help="with --skin: only the plain call's tactile map (a build without the flag can run it)")
    ap.add_argument("--stages", action="store_true", help="with --skin: only cast the tactile map `reps` times each way (for a kernel trace)")
    ap.add_argument("--parent-json", default=None, help="the result of another build (SOFTGRIP_LIB): its output digests are compared with this "
                    "run's, case by case; with --skin its plain tactile map figures are copied in under 'parent_build'")
    args = ap.parse_args()
    import torch
    import softgrip_amd as sg
    from softgrip_amd import native
    from softgrip_amd.create_dataset import episode_schedule
    from softgrip_amd.manenv import tactile_rays
    import render_ref as R
    if not torch.cuda.is_available():
        sys.exit("ray_bench.py needs a GPU: there is nothing to time without one")
    n = args.envs
    scene, damper, nstep = ("softball", "implicit", 20) if args.skin else ("softbox", "explicit", 100)
    m = sg.load_model(os.path.join(ROOT, "models", scene + ".sgmodel"), damper)
    nm = native.NativeModel(m)
    b = native.NativeBatch(nm, n, 0)
    if not args.skin:
        b.set_stiffness(np.random.RandomState(0).uniform(300, 1400, n), list(range(11, 64)), [0])
    flags = torch.zeros(n, dtype=torch.int32, device=b.device)
    sens = torch.zeros(n, nm.nsensordata, dtype=torch.float64, device=b.device)
    b.reset(1, sens=sens, flags=flags)
    sched = episode_schedule()
    for t in range(nstep):
        if sched[t] is not None:
            b.set_ctrl_broadcast(np.full(nm.nu, sched[t]))
        b.step(7, sens=sens, flags=flags)
    st = b.get_state()
    res = {"device": torch.cuda.get_device_name(0), "scene": scene, "state": "env step %d" % nstep, "envs": n, "ngeom": nm.ngeom, "reps": args.reps,
           "rounds": args.rounds, "method": "HIP events around `reps` back-to-back calls, median over `rounds` windows alternating with sg_step windows, ms per call",
           "library": "another build (SOFTGRIP_LIB)" if os.environ.get("SOFTGRIP_LIB") else "the tree's own build", "cases": []}

    def restore():
        b.set_state(qpos=st["qpos"], qvel=st["qvel"], act=st["act"], qacc_warmstart=st["qacc_warmstart"], ctrl=st["ctrl"])

    def measure(label, fn, layout=None, extra=None):
        os.environ.pop("SG_RAY_LAYOUT", None)
        if layout:
            os.environ["SG_RAY_LAYOUT"] = layout
        restore()
        fn()
        b.step(7, sens=sens, flags=flags)
        tr, ts = [], []
        for _ in range(args.rounds):
            restore()
            torch.cuda.synchronize()
            tr.append(window(torch, fn, args.reps))
            ts.append(window(torch, lambda: b.step(7, sens=sens, flags=flags), args.reps))
        restore()
        getattr(fn, "full", fn)()  # (once more on the sampled state, the normals written too, for the digest)
        sha = digest(torch, fn)
        os.environ.pop("SG_RAY_LAYOUT", None)
        case = {"case": label, "layout": layout or "automatic", "ms": float(np.median(tr)), "ms_windows": [float(x) for x in tr],
                "step_ms": float(np.median(ts)), "step_ms_windows": [float(x) for x in ts], "sha256": sha}
        case["over_step"] = case["ms"] / case["step_ms"]
        case.update(extra or {})
        res["cases"].append(case)
        print(json.dumps(case), flush=True)
        return case

    def caster(o, d, ids=None, **kw):
        """sg_ray into tensors made once (what a caller in a loop does): dist and geom ids"""
        k = n if ids is None else len(ids)
        nr = o.shape[-2]
        dist = torch.empty(k, nr, dtype=torch.float64, device=b.device)
        geom = torch.empty(k, nr, dtype=torch.int32, device=b.device)
        hb = kw.get("body")
        hb = None if hb is None else np.ascontiguousarray(hb, dtype=np.int32)
        import ctypes as C
        i32 = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
        hid = None if ids is None else np.ascontiguousarray(ids, dtype=np.int32)

        normal = torch.empty(k, nr, 3, dtype=torch.float64, device=b.device)

        def fn(nrm=None):
            b._check(b.L.sg_ray(b.ptr, i32(hid), k, nr, native._ptr(o), native._ptr(d), i32(hb), i32(hb), int(kw.get("cat_mask", 31)),
                                float(kw.get("max_dist", 0.0)), int(kw.get("flags", 0)), native._ptr(dist), native._ptr(geom), nrm, b._stream()))
        fn.dist, fn.geom = dist, geom
        fn.full, fn.outputs = (lambda: fn(native._ptr(normal))), (dist, geom, normal)     # (the timed call writes no normals; the hashed one does)
        return fn

    dev = b.device
    if args.skin:
        skin_cases(args, res, m, nm, b, torch, native, tactile_rays, measure, caster)
        return
    # (a) the tactile map's rays
    tr = tactile_rays(m, (8, 8))
    fa = caster(torch.tensor(tr["origin"].reshape(-1, 3), device=dev), torch.tensor(tr["direction"].reshape(-1, 3), device=dev), body=tr["body"].reshape(-1),
                cat_mask=native.SG_RAY_ELEM | native.SG_RAY_CENTER, max_dist=float(tr["thickness"].max()) + 0.05)
    for lay in (None, "rays", "geoms"):
        c = measure("(a) tactile_depth rays 8x8, %d rays per env" % tr["body"].size, fa, lay)
        c["hit_fraction"] = float((fa.geom >= 0).float().mean())
    # (b), (c): world-frame rays of the test recipe on env 0's poses
    import ray_ref as RR
    gx = b.poses([0])["geom_xpos"][0].cpu().numpy()
    o, d = RR.scene_rays(gx, np.asarray(m.geom_type), 1024, 3)
    ot, dt = torch.tensor(o, device=dev), torch.tensor(d, device=dev)
    measure("(b) one world-frame ray per env", caster(ot[:1].contiguous(), dt[:1].contiguous()))
    sweep = {}
    for nr in (1, 4, 16, 64, 256, 1024):
        for lay in ("rays", "geoms"):
            f = caster(ot[:nr].contiguous(), dt[:nr].contiguous())
            sweep[(nr, lay)] = measure("(c) %d world-frame rays per env" % nr, f, lay, {"n_rays": nr})["ms"]
    res["sweep_ms"] = {"%d" % nr: {lay: sweep[(nr, lay)] for lay in ("rays", "geoms")} for nr in (1, 4, 16, 64, 256, 1024)}
    res["geoms_layout_faster_up_to"] = max([nr for nr in (1, 4, 16, 64, 256, 1024) if sweep[(nr, "geoms")] < sweep[(nr, "rays")]], default=0)
    # (d) a camera's rays next to the renderer
    W, H, ids = 320, 240, list(range(16))
    cam = nm.default_camera()
    eye, f, dd = R.camera_rays(cam, W, H)
    fc = caster(torch.tensor(np.tile(eye, (W * H, 1)), device=dev), torch.tensor(dd.reshape(-1, 3), device=dev), ids=ids)
    depth = torch.empty(16, H, W, dtype=torch.float32, device=dev)
    hid = np.ascontiguousarray(ids, dtype=np.int32)
    import ctypes as C
    camp = np.ascontiguousarray(cam, dtype=np.float64)

    def fr():
        b._check(b.L.sg_render(b.ptr, camp.ctypes.data_as(C.POINTER(C.c_double)), hid.ctypes.data_as(C.POINTER(C.c_int32)), 16, W, H, None,
                               native._ptr(depth), None, b._stream()))
    cr = measure("(d) sg_ray, 16 envs x 320x240 camera rays", fc)
    cd = measure("(d) sg_render depth only, 16 envs x 320x240", fr)
    res["ray_over_render"] = cr["ms"] / cd["ms"]
    a_auto = [c for c in res["cases"] if c["case"].startswith("(a)") and c["layout"] == "automatic"][0]
    res["tactile_over_step"] = a_auto["over_step"]
    res["tactile_costs_less_than_one_step"] = a_auto["ms"] < a_auto["step_ms"]
    if args.parent_json:
        with open(args.parent_json) as f:
            bits_against(res, json.load(f))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fjson:
            json.dump(res, fjson, indent=1)
            fjson.write("\n")
    print("tactile map / one sg_step: %.3f; lanes-over-geoms faster up to %d rays per env; sg_ray / sg_render on camera rays: %.2f"
          % (res["tactile_over_step"], res["geoms_layout_faster_up_to"], res["ray_over_render"]))


def skin_cases(args, res, m, nm, b, torch, native, tactile_rays, measure, caster):
    """--skin: (a) the tactile map against capsules and skin, (b) the n_rays sweep with the flag, (c) the other build's plain figures"""
    import ray_ref as RR
    dev = b.device
    tr = tactile_rays(m, (8, 8))
    ta = dict(body=tr["body"].reshape(-1), cat_mask=native.SG_RAY_ELEM | native.SG_RAY_CENTER, max_dist=float(tr["thickness"].max()) + 0.05)
    to, td = torch.tensor(tr["origin"].reshape(-1, 3), device=dev), torch.tensor(tr["direction"].reshape(-1, 3), device=dev)
    label = "(a) tactile_depth rays 8x8, %d rays per env, " % tr["body"].size
    plain = caster(to, td, **ta)
    if args.stages:
        nm.set_skin(m.composite_skin())
        skin = caster(to, td, flags=native.SG_RAY_SKIN, **ta)
        for _ in range(args.reps):
            skin()
            plain()
        torch.cuda.synchronize()
        return
    for lay in (None, "rays", "geoms"):
        c = measure(label + "capsules (plain call)", plain, lay, {"skin": False})
        c["hit_fraction"] = float((plain.geom >= 0).float().mean())
    if not args.plain_only:
        if nm.skin() is None:
            nm.set_skin(m.composite_skin())
        res["skin"] = {"nvert": int(len(nm.skin()["vert_body"])), "nface": int(len(nm.skin()["face"]))}
        skin = caster(to, td, flags=native.SG_RAY_SKIN, **ta)
        for lay in (None, "rays", "geoms"):
            c = measure(label + "skin (SG_RAY_SKIN)", skin, lay, {"skin": True})
            c["hit_fraction"] = float((skin.geom >= 0).float().mean())
            c["skin_hit_fraction"] = float((skin.geom >= nm.ngeom).float().mean())
        gx = b.poses([0])["geom_xpos"][0].cpu().numpy()
        o, d = RR.scene_rays(gx, np.asarray(m.geom_type), 1024, 3)
        ot, dt = torch.tensor(o, device=dev), torch.tensor(d, device=dev)
        counts = (1, 4, 16, 32, 64, 128, 256, 1024)
        sweep = {}
        for nr in counts:
            for lay in ("rays", "geoms"):
                f = caster(ot[:nr].contiguous(), dt[:nr].contiguous(), flags=native.SG_RAY_SKIN)
                sweep[(nr, lay)] = measure("(b) %d world-frame rays per env, skin" % nr, f, lay, {"n_rays": nr, "skin": True})["ms"]
        res["sweep_ms"] = {"%d" % nr: {lay: sweep[(nr, lay)] for lay in ("rays", "geoms")} for nr in counts}
        res["geoms_layout_faster_up_to"] = max([nr for nr in counts if sweep[(nr, "geoms")] < sweep[(nr, "rays")]], default=0)
        auto = [c for c in res["cases"] if c["case"].startswith("(a)") and c["layout"] == "automatic"]
        res["skin_tactile_over_step"] = [c for c in auto if c["skin"]][0]["over_step"]
        res["skin_over_capsules"] = [c for c in auto if c["skin"]][0]["ms"] / [c for c in auto if not c["skin"]][0]["ms"]
    if args.parent_json:
        with open(args.parent_json) as f:
            parent = json.load(f)
        res["parent_build"] = {"what": "(c) the plain call's tactile map from the parent commit's build of the library, same session, same method",
                               "cases": [c for c in parent["cases"] if c["case"].startswith("(a)") and not c.get("skin")]}
        bits_against(res, parent)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fjson:
            json.dump(res, fjson, indent=1)
            fjson.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k not in ("cases", "parent_build")}))


if __name__ == "__main__":
    main()
