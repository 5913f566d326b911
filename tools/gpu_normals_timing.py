"""What vertex normals recomputed on the device cost (RayTraceRenderer.add_normals), against the bytes the two kernels move and against
what there was before: normals computed on the host and update_vertices with the result -- the same scene, the same process.

    python tools/gpu_normals_timing.py [--scenes small large] [--reps 7] [--repeats 5] [--bones 64] [--out profiles/normals_timing.txt]

The scene is the atrium, flattened, one normal set over every vertex: at its small detail (262 k triangles -- where k_skin, and so anything
like it, sits at the launch floor) and at 7.2 M triangles, which is where a rate means something.

  k_face_vectors, k_vertex_normals
                  each kernel alone (glz_debug_normals_timing: device events around 20 launches), `--repeats` times: min / median / max,
                  and the bytes the layout says one launch moves -- per face 12 of indices, 3 x 16 gathered, 16 out; per vertex 4 of row
                  length, 4 + 16 a row entry, 8 a slice, 32 in + 12 out -- over the median.  A GATHER's byte count is what the lanes ask
                  for, not what the memory system moves: the fraction of the streaming rate says how much of it the caches absorb.
  k_skin          THE YARDSTICK: the streaming kernel over the same vertex format, on a skin of `--bones` bones over the same vertices,
                  timed the same way in the same run (glz_debug_skin_timing), 88 bytes a vertex; its spread between repeats is what a
                  difference has to exceed to mean anything.
  pose            median wall time and update_ms of pose() with the set and without it, alternating phases: the added cost a frame.
  host            glz_host_vertex_normals on the host cores (its layout packer included: it has no handle to keep one in) plus
                  update_vertices with the result: what a caller with positions alone pays today.

After the timed calls the vertices are read back and compared with the host's, bit for bit.  One JSON line per measurement, then a table.

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
from glaze_amd.scenes import atrium_scene  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tools"))
from gpu_skin_timing import BYTES_PER_VERTEX as SKIN_BYTES_PER_VERTEX, chain, twist  # noqa: E402


def spread(values):
    return {"min": min(values), "median": statistics.median(values), "max": max(values)}


def timed_poses(r, scene, skin, bones, reps):
    r.pose({skin: bones[0]})                                                                      # (the first refit makes the plan: not timed)
    wall, stream = [], []
    for i in range(reps):
        t0 = time.perf_counter()
        r.pose({skin: bones[i % 2]})
        wall.append((time.perf_counter() - t0) * 1e3)
        stream.append(float(scene.info().build_ms))                                                # = glz_geometry_update_info::update_ms
    return statistics.median(wall), statistics.median(stream)


def measure(emit, inst, name, desc, args):
    inst.set_as_levels("flat")
    try:
        scene = glaze_amd.RayTraceScene.from_desc(inst, desc)
    finally:
        inst.set_as_levels("auto")
    r = glaze_amd.RayTraceRenderer.new(inst, scene, 64, 64)
    base = np.ascontiguousarray(desc.vertices).view(np.float32).reshape(-1, 8)
    n = base.shape[0]
    joints, sw, axis, centre = chain(desc.vertices, args.bones)
    bones = [twist(args.bones, axis, centre, a) for a in (0.05, -0.03)]
    skin = r.add_skin(0, joints, sw, args.bones)
    without = timed_poses(r, scene, skin, bones, args.reps)
    t0 = time.perf_counter()
    ns = r.add_normals(0, n)
    add_ms = (time.perf_counter() - t0) * 1e3
    face_ms, vertex_ms, skin_ms = [], [], []
    nbytes = (0, 0)
    for _ in range(args.repeats):                                                                 # the three take turns
        skin_ms.append(r.debug_skin_timing(skin, bones[0], reps=20))
        (f, v), nbytes = r.debug_normals_timing(ns, reps=20)
        face_ms.append(f)
        vertex_ms.append(v)
    with_set = timed_poses(r, scene, skin, bones, args.reps)
    r.pose({skin: bones[0]})
    posed = glaze_amd.host_skin(base, joints, sw, bones[0])
    t0 = time.perf_counter()
    want = posed.copy()
    want[:] = glaze_amd.host_vertex_normals(posed, desc.indices, desc.meshes, 0, n)
    host_ms = (time.perf_counter() - t0) * 1e3
    same = bool(np.array_equal(r.read_vertices(0, n).view(np.uint32), want.view(np.uint32)))
    r.remove_normals(ns)
    wall = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        r.update_vertices(want, first=0)
        wall.append((time.perf_counter() - t0) * 1e3)
    update_ms = statistics.median(wall)
    kf, kv, ks = spread(face_ms), spread(vertex_ms), spread(skin_ms)
    n_faces, skin_bytes = nbytes[0] // 76, SKIN_BYTES_PER_VERTEX * n
    rate = lambda b, ms: b / (ms * 1e-3) / 1e12   # noqa: E731
    row = {"scene": name, "vertices": n, "faces": int(n_faces), "row_entries": int((nbytes[1] - n * 48 - ((n + 63) // 64) * 8) // 20),
           "k_face_vectors_ms": kf, "k_face_vectors_bytes": nbytes[0], "k_face_vectors_TB_per_s": rate(nbytes[0], kf["median"]),
           "k_vertex_normals_ms": kv, "k_vertex_normals_bytes": nbytes[1], "k_vertex_normals_TB_per_s": rate(nbytes[1], kv["median"]),
           "k_skin_ms": ks, "k_skin_bytes": skin_bytes, "k_skin_TB_per_s": rate(skin_bytes, ks["median"]),
           "k_skin_TB_per_s_spread": [rate(skin_bytes, ks[k]) for k in ("max", "min")],
           "face_fraction_of_k_skin_rate": rate(nbytes[0], kf["median"]) / rate(skin_bytes, ks["median"]),
           "vertex_fraction_of_k_skin_rate": rate(nbytes[1], kv["median"]) / rate(skin_bytes, ks["median"]),
           "pose_wall_ms_without_set": without[0], "pose_update_ms_without_set": without[1], "pose_wall_ms_with_set": with_set[0], "pose_update_ms_with_set": with_set[1],
           "add_normals_wall_ms": add_ms, "host_vertex_normals_ms": host_ms, "update_vertices_wall_ms": update_ms, "posed_equals_host": same}
    emit(json.dumps(row))
    emit("")
    emit("%s: %d vertices, %d faces, %d row entries" % (name, n, row["faces"], row["row_entries"]))
    emit("")
    emit("| kernel | ms, min / median / max | bytes a launch | TB/s at the median | of k_skin's rate |")
    emit("|---|---|---|---|---|")
    emit("| k_face_vectors | %.4f / %.4f / %.4f | %d | %.2f | %.2f |" % (kf["min"], kf["median"], kf["max"], nbytes[0], row["k_face_vectors_TB_per_s"], row["face_fraction_of_k_skin_rate"]))
    emit("| k_vertex_normals | %.4f / %.4f / %.4f | %d | %.2f | %.2f |" % (kv["min"], kv["median"], kv["max"], nbytes[1], row["k_vertex_normals_TB_per_s"],
                                                                         row["vertex_fraction_of_k_skin_rate"]))
    emit("| k_skin (yardstick) | %.4f / %.4f / %.4f | %d | %.2f (%.2f .. %.2f) | 1 |" % (ks["min"], ks["median"], ks["max"], skin_bytes, row["k_skin_TB_per_s"],
                                                                                       *row["k_skin_TB_per_s_spread"]))
    emit("")
    emit("| | wall (ms) | update_ms |")
    emit("|---|---|---|")
    emit("| pose, no set | %.3f | %.3f |" % without)
    emit("| pose, a set over every vertex | %.3f | %.3f |" % with_set)
    emit("| host_vertex_normals, then update_vertices | %.1f + %.3f | |" % (host_ms, update_ms))
    emit("| add_normals, once | %.1f | |" % add_ms)
    emit("| the device's normals equal the host's, bit for bit | %s | |" % ("yes" if same else "NO"))
    emit("")
    del r, scene


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", nargs="+", default=["small", "large"])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--bones", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "normals_timing.txt"))
    args = ap.parse_args()
    lines = []

    def emit(text):
        print(text, flush=True)
        lines.append(text)

    inst = glaze_amd.RayTraceInstance.new()
    if "small" in args.scenes:
        measure(emit, inst, "atrium 262 k", atrium_scene(texture_size=256, sky_size=(512, 256)), args)
    if "large" in args.scenes:
        measure(emit, inst, "atrium 7.2 M", atrium_scene(detail=16.0, texture_size=256, sky_size=(512, 256)), args)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
