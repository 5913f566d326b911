"""What moving the instances costs (RayTraceRenderer.update_transforms) against creating the scene again, on forest_scene(n).

    python tools/gpu_update_timing.py [--n 1000 10000 50000] [--reps 5]

Per n and shape (flattened / two levels): the median wall time of update_transforms (alternating two transform sets), of creating
the scene again and of the host box rule alone (the loop two-level creation runs), and the median device-event time of the two box
kernels in the updates (glz_debug_box_kernel_ms).  A last row takes the other shape of load: one mesh of 1 M vertices instanced 8
times.  The flattened shape stops at 10 000 columns (50 000 would be 307 M world triangles).  A separate run under
`rocprofv3 --kernel-trace --stats` cross-checks the kernel times.  One JSON line per row, then a markdown table.
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
from glaze_amd.scene_desc import INSTANCE_DTYPE, MESH_DTYPE, VERTEX_DTYPE, SceneDesc  # noqa: E402
from glaze_amd.scenes import forest_scene  # noqa: E402


def ms(f, reps):
    out = []
    for i in range(reps):
        t0 = time.perf_counter()
        f(i)
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def big_mesh_scene(side=1024, copies=8):
    """one wavy grid of side x side vertices (2 M triangles) under `copies` rotated placements"""
    y, x = np.mgrid[0:side, 0:side].astype(np.float32) / np.float32(side - 1)
    v = np.zeros(side * side, VERTEX_DTYPE)
    v["vv"] = np.stack([x.ravel(), 0.05 * np.sin(12 * x.ravel()) * np.cos(9 * y.ravel()), y.ravel()], 1)
    q = (np.arange(side - 1)[:, None] * side + np.arange(side - 1)[None, :]).ravel()
    idx = np.stack([q, q + side, q + 1, q + 1, q + side, q + side + 1], 1).astype(np.uint32).ravel()
    rng = np.random.default_rng(5)
    mats = []
    for i in range(copies):
        a = rng.uniform(0, 2 * np.pi)
        m = np.eye(4)
        m[:3, :3] = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        m[:3, 3] = (2.0 * i, 0.0, 0.0)
        mats.append(np.asarray(m, np.float32).T.reshape(16))
    return SceneDesc(v, idx, np.array([(0, 0, 0, idx.size)], MESH_DTYPE), np.stack(mats),
                     np.array([(0, i) for i in range(copies)], INSTANCE_DTYPE))


def moved(desc, seed):
    t = desc.transforms.copy().reshape(-1, 4, 4)
    rng = np.random.default_rng(seed)
    t[1:, 3, 0] += rng.uniform(-1, 1, t.shape[0] - 1).astype(np.float32)
    t[1:, 3, 2] += rng.uniform(-1, 1, t.shape[0] - 1).astype(np.float32)
    return t.reshape(-1, 16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[1000, 10000, 50000])
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    inst = glaze_amd.RayTraceInstance.new()
    rows = []
    cases = [("forest", n, forest_scene(n)) for n in args.n] + [("1M-vertex mesh", 8, big_mesh_scene())]
    for name, n, desc in cases:
        sets = [desc.transforms, moved(desc, 1)]
        for levels in ("flat", "two_level"):
            if levels == "flat" and (n > 10000 or name != "forest"):
                continue
            inst.set_as_levels(levels)
            scene = glaze_amd.RayTraceScene.from_desc(inst, desc)
            r = glaze_amd.RayTraceRenderer.new(inst, scene, 64, 64)
            r.update_transforms(sets[1])                                          # first update builds the device points
            row = {"scene": name, "n": n, "levels": levels, "instances": int(desc.instances.shape[0])}
            kernel = []

            def update(i):
                r.update_transforms(sets[i % 2])
                kernel.append(scene.debug_box_kernel_ms())
            row["update_ms"] = ms(update, args.reps)
            row["update_build_ms"] = float(scene.info().build_ms)
            row["create_ms"] = ms(lambda i: glaze_amd.RayTraceScene.from_desc(inst, desc), max(1, args.reps // 2))
            if levels == "two_level":
                row["host_boxes_ms"] = ms(lambda i: scene.debug_instance_boxes(False), args.reps)
                row["box_kernel_ms"] = statistics.median(kernel)
            inst.set_as_levels("auto")
            del r, scene
            print(json.dumps(row), flush=True)
            rows.append(row)
    print("| scene | instances | shape | update_transforms (ms) | of which on the stream (ms) | create again (ms) | host box rule (ms) | box kernels (ms) |")
    print("|---|---|---|---|---|---|---|---|")
    for r in rows:
        f = lambda k: ("%.3f" % r[k]) if k in r else "-"  # noqa: E731
        print("| %s | %d | %s | %s | %s | %s | %s | %s |" % (r["scene"], r["instances"], r["levels"], f("update_ms"), f("update_build_ms"),
                                                        f("create_ms"), f("host_boxes_ms"), f("box_kernel_ms")))


if __name__ == "__main__":
    main()
