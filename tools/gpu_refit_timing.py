"""What deforming a mesh costs (RayTraceRenderer.update_vertices) in both modes against creating the scene again, and what a refitted
tree costs to trace.

    python tools/gpu_refit_timing.py [--scenes small large forest] [--forest-n 1000] [--reps 5] [--amplitudes 0.02 0.1 0.5]

Scenes: the atrium at its small detail (262 k triangles) and at 7.2 M triangles, every vertex on a wave (flattened, a full-range
update); forest_scene(n) in two levels with the column mesh bent (its vertex range alone is updated).  Per scene: the median wall time
and the median stream time (glz_geometry_update_info::update_ms = glz_scene_info::build_ms) of update_vertices in mode refit, alternating two vertex sets, the same
in mode rebuild, and the median wall time of creating the scene again -- the only way there was before.  The first refit, which makes
the refit plan and takes the built tree's box-area figure, is timed on its own.  Then, per deformation amplitude (in units of the wave's
own length scale), a scene refitted from rest to that amplitude: box_area / box_area_built, and the time of 24 launches at 1280 x 720
on it against the same on a scene built fresh with those vertices.  One JSON line per row, then markdown tables.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import glaze_amd  # noqa: E402
from glaze_amd.scenes import atrium_scene, forest_scene  # noqa: E402


def ms(f, reps):
    out = []
    for i in range(reps):
        t0 = time.perf_counter()
        f(i)
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def waved(desc, first, count, amp, scale):
    """vertices [first, first + count) with a wave of height amp * scale and wavelength ~ 6 scale across x and z"""
    v = desc.vertices[first:first + count].copy()
    p = v["vv"].astype(np.float64)
    p[:, 1] += amp * scale * np.sin(p[:, 0] / scale) * np.cos(p[:, 2] / scale)
    p[:, 0] += 0.5 * amp * scale * np.sin(p[:, 1] / scale)
    v["vv"] = p.astype(np.float32)
    return v


def render_ms(r, launches=24, reps=3):
    def once(_):
        r.restart()
        r.step(launches)
        r.wait_idle()
    once(0)
    return ms(once, reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", nargs="+", default=["small", "large", "forest"])
    ap.add_argument("--forest-n", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--amplitudes", type=float, nargs="+", default=[0.02, 0.1, 0.5])
    args = ap.parse_args()
    inst = glaze_amd.RayTraceInstance.new()
    cases = []
    if "small" in args.scenes:
        d = atrium_scene(texture_size=256, sky_size=(512, 256))
        cases.append(("atrium 262 k", d, "flat", 0, d.vertices.shape[0], 1.0))
    if "large" in args.scenes:
        d = atrium_scene(detail=16.0, texture_size=256, sky_size=(512, 256))
        cases.append(("atrium 7.2 M", d, "flat", 0, d.vertices.shape[0], 1.0))
    if "forest" in args.scenes:
        d = forest_scene(args.forest_n)
        m = d.meshes[1]                                                                           # the column
        used = d.indices[int(m["index_offset"]):int(m["index_offset"]) + int(m["index_count"])]
        cases.append(("forest %d, column bent" % args.forest_n, d, "two_level", int(used.min()), int(used.max() - used.min() + 1), 0.3))
    timing, quality = [], []
    for name, desc, levels, first, count, scale in cases:
        def create(vertices=None):
            dd = desc
            if vertices is not None:
                dd = desc.copy()
                dd.vertices[first:first + count] = vertices
            inst.set_as_levels(levels)
            try:
                return glaze_amd.RayTraceScene.from_desc(inst, dd)
            finally:
                inst.set_as_levels("auto")
        sets = [desc.vertices[first:first + count].copy(), waved(desc, first, count, 0.1, scale)]
        scene = create()
        r = glaze_amd.RayTraceRenderer.new(inst, scene, 64, 64)
        i = scene.info()
        leaves = int(glaze_amd.abi.lib().glz_debug_read_leaf_records(scene._h, None, 0))
        row = {"scene": name, "levels": levels, "triangles": int(i.n_as_triangles), "vertices_updated": count, "as_bytes": int(i.as_bytes),
               # the refit plan: a box per leaf, a box and a place in the level lists per wide node (two levels: the top level's nodes have none)
               "plan_bytes": 32 * leaves + 36 * (int(i.bvh_nodes) + int(i.bvh_nodes8))}
        t0 = time.perf_counter()
        r.update_vertices(sets[1], first=first)
        row["first_refit_ms"] = (time.perf_counter() - t0) * 1e3
        for mode in ("refit", "rebuild"):
            stream = []

            def update(i):
                r.update_vertices(sets[i % 2], first=first, mode=mode)
                stream.append(float(scene.info().build_ms))    # = update_ms (asking for geometry_update_info after a rebuild would make the refit plan)
            row[mode + "_ms"] = ms(update, args.reps)
            row[mode + "_stream_ms"] = statistics.median(stream)
        row["create_ms"] = ms(lambda i: create(), max(2, args.reps // 2))
        del r, scene
        print(json.dumps(row), flush=True)
        timing.append(row)
        for amp in args.amplitudes:
            v = waved(desc, first, count, amp, scale)
            a, b = create(), create(v)
            ra, rb = (glaze_amd.RayTraceRenderer.new(inst, s, 1280, 720) for s in (a, b))
            ra.update_vertices(v, first=first)
            u = ra.geometry_update_info()
            q = {"scene": name, "amplitude": amp, "box_area_ratio": u.box_area / u.box_area_built if u.box_area_built else float("nan"),
                 "refitted_render_ms": render_ms(ra), "fresh_render_ms": render_ms(rb)}
            del ra, rb, a, b
            print(json.dumps(q), flush=True)
            quality.append(q)
    print("| scene | shape | triangles | vertices updated | first refit (ms) | refit (ms) | on the stream (ms) | rebuild (ms) | on the stream (ms) | create again (ms) | plan / structure (MB) |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for r in timing:
        print("| %s | %s | %d | %d | %.3f | %.3f | %.3f | %.3f | %.3f | %.3f | %.1f / %.1f |" % (
            r["scene"], r["levels"], r["triangles"], r["vertices_updated"], r["first_refit_ms"], r["refit_ms"], r["refit_stream_ms"], r["rebuild_ms"],
            r["rebuild_stream_ms"], r["create_ms"], r["plan_bytes"] / 1e6, r["as_bytes"] / 1e6))
    print()
    print("| scene | amplitude | box_area / box_area_built | 24 launches, refitted (ms) | 24 launches, built fresh (ms) |")
    print("|---|---|---|---|---|")
    for q in quality:
        print("| %s | %g | %.3f | %.3f | %.3f |" % (q["scene"], q["amplitude"], q["box_area_ratio"], q["refitted_render_ms"], q["fresh_render_ms"]))


if __name__ == "__main__":
    main()
