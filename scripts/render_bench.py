"""Headless renderer timings (HIP events) on the GPU: sg_render as a whole, its pose/record kernel alone (sg_render with no image output
runs only sg_kin_kernel) and so the ray-casting kernel by difference, and the cost of rendering inside an env step loop.

  1. 4096 envs x 64 x 64, depth + segid      2. 16 envs x 640 x 480, rgba
  3. softbox env step (7 substeps, 4096 envs) with 4 envs rendered at 320 x 240 after every step, against the same step alone

The FP32 share is an ESTIMATE: rays x the mean culled list length per tile (the kernel's cone test restated in NumPy on the envs'
poses) x ~60 FLOP per ray - primitive test, against 157.3 TFLOP/s.

--windows N repeats every timing in N windows of --reps calls and records each window (their spread is what a second build's time is
held against).  --skin adds the skin path (sg_render_ex with SG_RENDER_SKIN, the skin from Model.composite_skin()): the whole call,
its pose + vertex stage alone (no image output) and so sg_rskin_kernel by difference, with the mean culled list lengths per tile
(geoms the skin does not replace, triangles) restated in NumPy.

usage: python scripts/render_bench.py [--scene softbox] [--reps 20] [--tendon-damper implicit] [--windows 1] [--skin] [--label TEXT] [--out profiles/r06_render_bench.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FLOP_PER_TEST = 60.0
PEAK_FP32 = 157.3e12


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
    """n windows of `reps` calls: dict with every window's mean (ms), their median, min and max"""
    w = [timed(torch, fn, reps) for _ in range(n)]
    return {"windows_ms": w, "median_ms": float(np.median(w)), "min_ms": min(w), "max_ms": max(w)}


def mean_list_length(nm, batch, cam, w, h, envs, skin=None):
    """the kernel's tile cull (sg_render.h sgr_tile_cone / sgr_cone_keep) restated in fp64 on the listed envs' poses; with a skin: the
    pair (geoms the skin does not replace, triangles by sgr_tri_cone_keep's bounding sphere about the centroid)"""
    import render_ref as R
    p = batch.poses(envs)
    m = nm.model
    if skin is not None:
        import skin_ref as S
        from softgrip_amd.mjcf import quat_to_mat
        shown = ~S.hidden_geoms(m, skin)
        face = np.asarray(skin["face"])
        tris = []
    eye, f, d = R.camera_rays(cam, w, h)
    s = np.asarray(m.geom_size)
    t = np.asarray(m.geom_type)
    rb = np.where(t == 2, s[:, 0], np.where(t == 3, s[:, 0] + s[:, 1], np.where(t == 6, np.linalg.norm(s, axis=1), np.inf)))
    out = []
    for k in range(len(envs)):
        c = p["geom_xpos"][k].cpu().numpy() - eye
        if skin is not None:
            xmat = np.array([quat_to_mat(q) for q in p["xquat"][k].cpu().numpy()])
            v = S.skin_vertices(skin, p["xpos"][k].cpu().numpy(), xmat)[face] - eye      # [nface, 3, 3]
            tc = v.mean(1)
            tr = np.linalg.norm(v - tc[:, None], axis=2).max(1)
        for j0 in range(0, h, 16):
            for i0 in range(0, w, 16):
                j1, i1 = min(j0 + 15, h - 1), min(i0 + 15, w - 1)
                cd = np.stack([d[j0, i0], d[j0, i1], d[j1, i0], d[j1, i1]])
                ax = cd.sum(0)
                ax /= np.linalg.norm(ax)
                cs = (cd @ ax).min()
                sn = np.sqrt(max(0.0, 1 - cs * cs))
                a = c @ ax
                perp = np.linalg.norm(c - a[:, None] * ax, axis=1)
                keep = (perp * cs - a * sn <= rb) | ~np.isfinite(rb)
                if skin is None:
                    out.append(int(keep.sum()))
                    continue
                out.append(int((keep & shown).sum()))
                ta = tc @ ax
                tris.append(int((np.linalg.norm(tc - ta[:, None] * ax, axis=1) * cs - ta * sn <= tr).sum()))
    return float(np.mean(out)) if skin is None else (float(np.mean(out)), float(np.mean(tris)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="softbox")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--tendon-damper", default=None, choices=["explicit", "implicit"], help="softball / softcylinder need implicit (DESIGN.md D5)")
    ap.add_argument("--windows", type=int, default=1)
    ap.add_argument("--skin", action="store_true")
    ap.add_argument("--label", default=None, help="free text stored in the result (which build this is)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import softgrip_amd as sg
    from softgrip_amd import native
    m = sg.load_model(os.path.join(ROOT, "models", args.scene + ".sgmodel"), args.tendon_damper)
    nm = native.NativeModel(m)
    res = {"scene": args.scene, "ngeom": nm.ngeom, "nbody": nm.nbody, "device": torch.cuda.get_device_name(0), "reps": args.reps,
           "flop_per_ray_primitive_test_estimate": FLOP_PER_TEST, "peak_fp32_tflops": PEAK_FP32 / 1e12, "cases": []}
    if args.label:
        res["label"] = args.label
    if args.windows > 1:
        res["windows"] = args.windows
    skin = m.composite_skin() if args.skin else None
    b = native.NativeBatch(nm, 4096, 0)
    b.reset(1)
    b.set_ctrl_broadcast(np.full(nm.nu, -0.2))
    for _ in range(20):
        b.step(7)
    cam = nm.default_camera()
    res["state_finite"] = bool(torch.isfinite(b.get_state()["qpos"]).all())      # (a NaN env renders as background: timings of it mean nothing)

    def case(name, n, w, h, rgb, depth, seg):
        ids = list(range(n))
        outs = b.render(cam, ids, w, h, rgb=rgb, depth=depth, seg=seg)   # (allocates the outputs once)
        L, ptr = b.L, b.ptr
        import ctypes as C
        cp = (C.c_double * 7)(*cam)
        ia = (C.c_int32 * n)(*ids)
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        p = lambda k: C.c_void_p(outs[k].data_ptr()) if k in outs else None  # noqa: E731
        full = timed(torch, lambda: native.check(L.sg_render(ptr, cp, ia, n, w, h, p("rgba"), p("depth"), p("seg"), st), L), args.reps)
        fk = timed(torch, lambda: native.check(L.sg_render(ptr, cp, ia, n, w, h, None, None, None, st), L), args.reps)
        rays = n * w * h
        ml = mean_list_length(nm, b, cam, w, h, ids[:4])
        ray_ms = max(full - fk, 1e-9)
        flops = rays * ml * FLOP_PER_TEST
        r = {"case": name, "envs": n, "width": w, "height": h, "outputs": [k for k in ("rgba", "depth", "seg") if k in outs],
             "ms_sg_render": full, "ms_sg_kin_kernel": fk, "ms_sg_render_kernel": full - fk, "rays": rays,
             "rays_per_s": rays / (full * 1e-3), "mean_culled_list_per_tile_estimate": ml,
             "render_kernel_fp32_share_of_peak_estimate": flops / (ray_ms * 1e-3) / PEAK_FP32,
             "dominant_kernel": "sg_render_kernel" if full - fk > fk else "sg_kin_kernel"}
        if args.windows > 1:
            r["sg_render_windows"] = windows(torch, lambda: native.check(L.sg_render(ptr, cp, ia, n, w, h, p("rgba"), p("depth"), p("seg"), st), L), args.reps, args.windows)
        res["cases"].append(r)
        print(json.dumps(r), flush=True)
        if skin is None:
            return
        nm.set_skin(skin)
        ex = lambda *o: native.check(L.sg_render_ex(ptr, cp, ia, n, w, h, native.SG_RENDER_SKIN, *o, st), L)  # noqa: E731
        sfull = windows(torch, lambda: ex(p("rgba"), p("depth"), p("seg")), args.reps, args.windows)
        spre = windows(torch, lambda: ex(None, None, None), args.reps, args.windows)
        mg, mt = mean_list_length(nm, b, cam, w, h, ids[:4], skin)
        seg = b.render(cam, ids[:4], w, h, rgb=False, depth=False, seg=True, skin=True)["seg"]
        r = {"case": name + ", skin", "envs": n, "width": w, "height": h, "outputs": [k for k in ("rgba", "depth", "seg") if k in outs],
             "nvert": len(skin["vert_body"]), "nface": len(skin["face"]), "sg_render_ex": sfull, "sg_kin_kernel_plus_sg_skin_vert_kernel": spre,
             "ms_sg_rskin_kernel": sfull["median_ms"] - spre["median_ms"], "rays_per_s": rays / (sfull["median_ms"] * 1e-3),
             "mean_culled_geoms_per_tile_estimate": mg, "mean_culled_triangles_per_tile_estimate": mt,
             "skin_pixel_fraction": float((seg == nm.ngeom).float().mean()),
             "skin_over_plain": sfull["median_ms"] / (r["sg_render_windows"]["median_ms"] if args.windows > 1 else full)}
        nm.set_skin(None)
        res["cases"].append(r)
        print(json.dumps(r), flush=True)

    case("4096 envs x 64x64 depth+segid", 4096, 64, 64, False, True, True)
    case("16 envs x 640x480 rgba", 16, 640, 480, True, False, False)
    if args.skin:      # (the step-loop case is the plain renderer's: r06)
        if args.out:
            with open(args.out, "w") as f:
                json.dump(res, f, indent=1)
        return
    sens = torch.zeros(4096, nm.nsensordata, dtype=torch.float64, device=b.device)
    plain = timed(torch, lambda: b.step(7, sens=sens), args.reps)
    with_r = timed(torch, lambda: (b.step(7, sens=sens), b.render(cam, [0, 1, 2, 3], 320, 240)), args.reps)
    r = {"case": "env step (4096 envs, 7 substeps) + render 4 envs 320x240 after every step", "ms_step": plain, "ms_step_plus_render": with_r,
         "render_overhead_ms": with_r - plain, "render_overhead_fraction": (with_r - plain) / plain}
    res["cases"].append(r)
    print(json.dumps(r), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
