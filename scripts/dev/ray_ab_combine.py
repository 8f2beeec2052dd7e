"""usage: ray_ab_combine.py DIR OUT.json -- DIR holds {plain,skin}_{parent1,new,parent2}.json: the
parent / new / parent runs of scripts/ray_bench.py (plain and --skin) -> one file: per figure the new build's windows and median, the
parent's windows of both runs, the slowest of them (the bound) and whether the new median is within it; the output digests' verdicts"""
import json
import os
import sys

out = {"what": "scripts/ray_bench.py and scripts/ray_bench.py --skin, in the order parent, new, parent, each in a process of its own, one visit of one "
               "MI355X; the parent is the parent commit's build of the library (SOFTGRIP_LIB).  Bound per figure: the slowest window the parent "
               "itself produced, pooled over its two runs; the new build's median must not exceed it.  Put together by scripts/dev/ray_ab_combine.py.  sha256: of dist | geom ids | normals of one more call "
               "on the sampled state", "runs": {}, "figures": [], "bits": {}}
worst, control = 0, []
for mode in ("plain", "skin"):
    runs = {k: json.load(open(os.path.join(sys.argv[1], "%s_%s.json" % (mode, k)))) for k in ("parent1", "new", "parent2")}
    out["runs"][mode] = {k: {kk: v for kk, v in r.items() if kk not in ("cases", "bits_vs_parent", "parent_build")} for k, r in runs.items()}
    out["bits"][mode] = {"new against parent": runs["new"]["bits_vs_parent"], "parent against parent (control)": runs["parent2"]["bits_vs_parent"]}
    for cn, c1, c2 in zip(runs["new"]["cases"], runs["parent1"]["cases"], runs["parent2"]["cases"]):
        assert (cn["case"], cn["layout"]) == (c1["case"], c1["layout"]) == (c2["case"], c2["layout"])
        if cn["sha256"] is None:
            continue      # (sg_render beside the camera rays: not a ray query)
        pooled = c1["ms_windows"] + c2["ms_windows"]
        fig = {"mode": mode, "case": cn["case"], "layout": cn["layout"], "new_ms": cn["ms"], "new_ms_windows": cn["ms_windows"],
               "parent_ms": [c1["ms"], c2["ms"]], "parent_ms_windows": [c1["ms_windows"], c2["ms_windows"]], "bound_ms": max(pooled),
               "within": cn["ms"] <= max(pooled), "new_over_parent_median": cn["ms"] / (0.5 * (c1["ms"] + c2["ms"])),
               "step_ms": [c1["step_ms"], cn["step_ms"], c2["step_ms"]], "sha256": cn["sha256"], "sha256_parent": c1["sha256"]}
        out["figures"].append(fig)
        worst += not fig["within"]
        for x, y, name in ((c1, c2, "parent1 over parent2"), (c2, c1, "parent2 over parent1")):
            if x["ms"] > max(y["ms_windows"]):
                control.append({"mode": mode, "case": cn["case"], "layout": cn["layout"], "which": name, "median_ms": x["ms"], "other_slowest_ms": max(y["ms_windows"])})
        print("%-6s %-5s %-70s %-9s new %.4f parent %.4f / %.4f bound %.4f  x%.3f" % ("ok" if fig["within"] else "OVER", mode, cn["case"][:70], cn["layout"], cn["ms"],
                                                                                    c1["ms"], c2["ms"], max(pooled), fig["new_over_parent_median"]))
# the bound's own noise: one parent run's median held against the slowest window of the OTHER parent run alone (the same library twice)
out["control_parent_against_parent"] = {"what": "figures at which the median of one parent run exceeds the slowest window of the other parent run: the same "
                                                 "library in two processes", "over": control, "figures": len(out["figures"])}
print("control: %d of %d figures where one parent run's median is over the other's slowest window" % (len(control), 2 * len(out["figures"])))
out["figures_over_the_bound"] = worst
out["digests_different"] = sum(out["bits"][m]["new against parent"]["different"] for m in out["bits"])
json.dump(out, open(sys.argv[2], "w"), indent=1)
print("%d figures, %d over the bound, %d digests DIFFERENT" % (len(out["figures"]), worst, out["digests_different"]))
