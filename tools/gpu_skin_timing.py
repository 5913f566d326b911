"""What posing a skinned mesh on the device costs (RayTraceRenderer.pose) against what there was before: skinning on the host and
update_vertices with the posed vertices -- the same scene, the same vertices, the same process.

    python tools/gpu_skin_timing.py [--scenes small large forest] [--forest-n 1000] [--reps 7] [--bones 64] [--kernel-repeats 5]

Scenes: the atrium at its small detail (262 k triangles) and at 7.2 M triangles, every vertex skinned (flattened); forest_scene(n) in two
levels with the column mesh skinned (its vertex range alone).  The skeleton is a chain of `--bones` bones along the scene's longest axis,
each vertex under the two bones nearest to it (convex weights, the other two influences zero); two poses alternate, small rotations
about the chain's axis.  Per scene, in mode refit, once with the skin in linear mode and once in dual-quaternion mode (set_skin_blend; the
update_vertices side is then fed what glz_host_skin_dq makes), both in the same process:

  pose            median wall time around pose() (bones over the bus, k_skin, derivatives, refit), and the median update_ms of it;
  update_vertices median wall time around update_vertices() fed the vertices glz_host_skin made of the same bones BEFORE the clock starts
                  (the host's skinning time is given on its own and is in neither figure), and the median update_ms of it;
  k_skin          the kernel alone (glz_debug_skin_timing: device events around 20 launches), and its algorithmic bytes -- 88 a vertex:
                  32 bind + 8 joints + 16 weights in, 32 out -- over that time; k_skin_dq, which moves the same bytes, turn by turn with
                  it: --kernel-repeats measurements each, the median and the lowest and highest.

Both paths end in a wait for the stream, so the wall times are whole calls.  The two alternate call by call, so that what else the host
does falls on both.  After the timed calls the posed vertices are read back and compared with the host's, bit for bit.  One JSON line per
scene, then a markdown table.

The kernel names in the text, the table rows and the JSON keys -- k_skin, k_skin_dq, k_morph, k_morph_skin, k_morph_skin_dq -- name the RULE
a launch runs: each is a set of instantiations of one template, k_deform (kernels_deform.hip), and was a kernel of its own in earlier
result files, which therefore compare key for key.
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
    ap.add_argument("--kernel-repeats", type=int, default=5)
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
        skin = r.add_skin(first, joints, weights, args.bones)
        row = {"scene": name, "levels": levels, "vertices_skinned": count, "bones": args.bones, "k_skin_bytes": BYTES_PER_VERTEX * count}
        for blend, tag in (("linear", ""), ("dual_quaternion", "dq_")):
            r.set_skin_blend(skin, blend)
            t0 = time.perf_counter()
            posed = [glaze_amd.host_skin(bind, joints, weights, b, blend=blend) for b in poses]
            row[tag + "host_skin_ms"] = (time.perf_counter() - t0) * 1e3 / len(poses)
            r.update_vertices(posed[1], first=first)                                              # the first refit makes the plan: not timed
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
                stream[which].append(float(scene.info().build_ms))                                # = glz_geometry_update_info::update_ms
            r.pose({skin: poses[0]})
            row[tag + "posed_equals_host_skin"] = bool(np.array_equal(r.read_vertices(first, count).view(np.uint32), posed[0].view(np.uint32)))
            row.update({tag + "pose_wall_ms": statistics.median(wall["pose"]), tag + "pose_wall_min_max_ms": [min(wall["pose"]), max(wall["pose"])],
                        tag + "pose_update_ms": statistics.median(stream["pose"]),
                        tag + "update_vertices_wall_ms": statistics.median(wall["update"]),
                        tag + "update_vertices_wall_min_max_ms": [min(wall["update"]), max(wall["update"])],
                        tag + "update_vertices_update_ms": statistics.median(stream["update"])})
            row[tag + "wall_ratio"] = row[tag + "pose_wall_ms"] / row[tag + "update_vertices_wall_ms"]
        # the two kernels alone, turn by turn in one process: 20 launches between device events, --kernel-repeats times each, medians
        kernel = {"linear": [], "dual_quaternion": []}
        for _ in range(args.kernel_repeats):
            for blend in kernel:
                r.set_skin_blend(skin, blend)
                kernel[blend].append(r.debug_skin_timing(skin, poses[1], reps=20))
        for blend, tag in (("linear", "k_skin"), ("dual_quaternion", "k_skin_dq")):
            ms = statistics.median(kernel[blend])
            row.update({tag + "_ms": ms, tag + "_min_max_ms": [min(kernel[blend]), max(kernel[blend])],
                        tag + "_TB_per_s": BYTES_PER_VERTEX * count / (ms * 1e-3) / 1e12 if ms > 0 else float("nan")})
        row["k_skin_dq_over_k_skin"] = row["k_skin_dq_ms"] / row["k_skin_ms"]
        print(json.dumps(row), flush=True)
        rows.append(row)
        del r, scene
    print("| scene | shape | vertices skinned | blend | pose: wall (ms) | update_ms | update_vertices: wall (ms) | update_ms | pose / update_vertices (wall) | host skinning, not in either (ms) | kernel (ms, median) | min - max | 88 B a vertex over it (TB/s) | against k_skin | bits equal |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for w in rows:
        for blend, tag, k in (("linear", "", "k_skin"), ("dual quaternion", "dq_", "k_skin_dq")):
            print("| %s | %s | %d | %s | %.3f | %.3f | %.3f | %.3f | %.2f | %.1f | %.4f | %.4f - %.4f | %.2f | %.2f | %s |" % (
                w["scene"], w["levels"], w["vertices_skinned"], blend, w[tag + "pose_wall_ms"], w[tag + "pose_update_ms"], w[tag + "update_vertices_wall_ms"],
                w[tag + "update_vertices_update_ms"], w[tag + "wall_ratio"], w[tag + "host_skin_ms"], w[k + "_ms"], w[k + "_min_max_ms"][0], w[k + "_min_max_ms"][1],
                w[k + "_TB_per_s"], w[k + "_ms"] / w["k_skin_ms"], "yes" if w[tag + "posed_equals_host_skin"] else "NO"))


if __name__ == "__main__":
    main()
