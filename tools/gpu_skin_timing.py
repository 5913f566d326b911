"""What posing a skinned mesh on the device costs (RayTraceRenderer.pose) against what there was before: skinning on the host and
update_vertices with the posed vertices -- the same scene, the same vertices, the same process.

    python tools/gpu_skin_timing.py [--scenes small large forest] [--forest-n 1000] [--reps 7] [--bones 64]

Scenes: the atrium at its small detail (262 k triangles) and at 7.2 M triangles, every vertex skinned (flattened); forest_scene(n) in two
levels with the column mesh skinned (its vertex range alone).  The skeleton is a chain of `--bones` bones along the scene's longest axis,
each vertex under the two bones nearest to it (convex weights, the other two influences zero); two poses alternate, small rotations
about the chain's axis.  Per scene, in mode refit:

  pose            median wall time around pose() (bones over the bus, k_skin, derivatives, refit), and the median update_ms of it;
  update_vertices median wall time around update_vertices() fed the vertices glz_host_skin made of the same bones BEFORE the clock starts
                  (the host's skinning time is given on its own and is in neither figure), and the median update_ms of it;
  k_skin          the kernel alone (glz_debug_skin_timing: device events around 20 launches), and its algorithmic bytes -- 88 a vertex:
                  32 bind + 8 joints + 16 weights in, 32 out -- over that time.

Both paths end in a wait for the stream, so the wall times are whole calls.  The two alternate call by call, so that what else the host
does falls on both.  After the timed calls the posed vertices are read back and compared with the host's, bit for bit.  One JSON line per
scene, then a markdown table.
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

BYTES_PER_VERTEX = 32 + 8 + 16 + 32


def chain(vertices, n_bones):
    """joints and weights of a chain of n_bones bones along the longest axis of `vertices`, and the axis"""
    p = vertices["vv"].astype(np.float64)
    lo, hi = p.min(0), p.max(0)
    axis = int(np.argmax(hi - lo))
    s = (p[:, axis] - lo[axis]) / max(hi[axis] - lo[axis], 1e-9) * (n_bones - 1)
    b0 = np.clip(np.floor(s), 0, max(n_bones - 2, 0)).astype(np.int64)
    f = (s - b0).astype(np.float32) if n_bones > 1 else np.zeros(len(p), np.float32)
    b1 = np.minimum(b0 + 1, n_bones - 1)
    joints = np.stack([b0, b1, b0, b1], -1).astype(np.uint16)
    weights = np.stack([1.0 - f, f, np.zeros_like(f), np.zeros_like(f)], -1).astype(np.float32)
    centre = 0.5 * (lo + hi)
    return joints, weights, axis, centre


def twist(n_bones, axis, centre, angle):
    """bone k turns by angle * k / n about the chain's axis through `centre`: (n_bones, 16) float32, column-major"""
    out = []
    u, v = [a for a in range(3) if a != axis]
    for k in range(n_bones):
        a = angle * k / max(n_bones - 1, 1)
        m = np.eye(4)
        m[u, u], m[u, v], m[v, u], m[v, v] = np.cos(a), -np.sin(a), np.sin(a), np.cos(a)
        m[:3, 3] = centre - m[:3, :3] @ centre
        out.append(m.T.reshape(16))
    return np.asarray(out, np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", nargs="+", default=["small", "large", "forest"])
    ap.add_argument("--forest-n", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--bones", type=int, default=64)
    args = ap.parse_args()
    inst = glaze_amd.RayTraceInstance.new()
    cases = []
    if "small" in args.scenes:
        d = atrium_scene(texture_size=256, sky_size=(512, 256))
        cases.append(("atrium 262 k", d, "flat", 0, d.vertices.shape[0]))
    if "large" in args.scenes:
        d = atrium_scene(detail=16.0, texture_size=256, sky_size=(512, 256))
        cases.append(("atrium 7.2 M", d, "flat", 0, d.vertices.shape[0]))
    if "forest" in args.scenes:
        d = forest_scene(args.forest_n)
        m = d.meshes[1]                                                                           # the column
        used = d.indices[int(m["index_offset"]):int(m["index_offset"]) + int(m["index_count"])]
        cases.append(("forest %d, column skinned" % args.forest_n, d, "two_level", int(used.min()), int(used.max() - used.min() + 1)))
    rows = []
    for name, desc, levels, first, count in cases:
        inst.set_as_levels(levels)
        try:
            scene = glaze_amd.RayTraceScene.from_desc(inst, desc)
        finally:
            inst.set_as_levels("auto")
        r = glaze_amd.RayTraceRenderer.new(inst, scene, 64, 64)
        bind = desc.vertices[first:first + count]
        joints, weights, axis, centre = chain(bind, args.bones)
        poses = [twist(args.bones, axis, centre, a) for a in (0.05, -0.05)]
        t0 = time.perf_counter()
        posed = [glaze_amd.host_skin(bind, joints, weights, b) for b in poses]
        host_ms = (time.perf_counter() - t0) * 1e3 / len(poses)
        skin = r.add_skin(first, joints, weights, args.bones)
        r.update_vertices(posed[1], first=first)                                                  # the first refit makes the plan: not timed
        r.pose({skin: poses[0]})
        wall = {"pose": [], "update": []}
        stream = {"pose": [], "update": []}
        for i in range(2 * args.reps):
            k = (i // 2) % 2
            t0 = time.perf_counter()
            if i % 2 == 0:
                r.pose({skin: poses[k]})
            else:
                r.update_vertices(posed[1 - k], first=first)
            which = "pose" if i % 2 == 0 else "update"
            wall[which].append((time.perf_counter() - t0) * 1e3)
            stream[which].append(float(scene.info().build_ms))                                    # = glz_geometry_update_info::update_ms
        r.pose({skin: poses[0]})
        same = bool(np.array_equal(r.read_vertices(first, count).view(np.uint32), posed[0].view(np.uint32)))
        kernel_ms = r.debug_skin_timing(skin, poses[1], reps=20)
        row = {"scene": name, "levels": levels, "vertices_skinned": count, "bones": args.bones,
               "pose_wall_ms": statistics.median(wall["pose"]), "pose_wall_min_max_ms": [min(wall["pose"]), max(wall["pose"])],
               "pose_update_ms": statistics.median(stream["pose"]),
               "update_vertices_wall_ms": statistics.median(wall["update"]), "update_vertices_wall_min_max_ms": [min(wall["update"]), max(wall["update"])],
               "update_vertices_update_ms": statistics.median(stream["update"]),
               "host_skin_ms": host_ms, "k_skin_ms": kernel_ms, "k_skin_bytes": BYTES_PER_VERTEX * count,
               "k_skin_TB_per_s": BYTES_PER_VERTEX * count / (kernel_ms * 1e-3) / 1e12 if kernel_ms > 0 else float("nan"),
               "posed_equals_host_skin": same}
        row["wall_ratio"] = row["pose_wall_ms"] / row["update_vertices_wall_ms"]
        print(json.dumps(row), flush=True)
        rows.append(row)
        del r, scene
    print("| scene | shape | vertices skinned | pose: wall (ms) | update_ms | update_vertices: wall (ms) | update_ms | pose / update_vertices (wall) | host skinning, not in either (ms) | k_skin (ms) | 88 B a vertex over it (TB/s) | bits equal |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|")
    for w in rows:
        print("| %s | %s | %d | %.3f | %.3f | %.3f | %.3f | %.2f | %.1f | %.4f | %.2f | %s |" % (
            w["scene"], w["levels"], w["vertices_skinned"], w["pose_wall_ms"], w["pose_update_ms"], w["update_vertices_wall_ms"], w["update_vertices_update_ms"],
            w["wall_ratio"], w["host_skin_ms"], w["k_skin_ms"], w["k_skin_TB_per_s"], "yes" if w["posed_equals_host_skin"] else "NO"))


if __name__ == "__main__":
    main()
