"""What morph targets on the device cost (RayTraceRenderer.animate), against the bytes the kernels move and against what there was before:
blending on the host and update_vertices with the result -- the same scene, the same vertices, the same process.

    python tools/gpu_morph_timing.py [--scenes small large] [--reps 7] [--repeats 5] [--bones 64] [--out profiles/morph_timing.txt]

The scene is the atrium, flattened, every vertex morphed: at its small detail (262 k triangles, 141 k vertices -- where k_skin, and so
anything like it, sits at the launch floor) and at 7.2 M triangles (3.6 M vertices), which is where a rate means something.  Two sets of
targets, random small deltas: "8 dense" (eight targets without index lists) and, on the small scene, "50 sparse" (fifty targets that each
touch a random tenth of the vertices, so a row holds five entries on average and a slice is as wide as its longest row).

  k_morph         the kernel alone (glz_debug_morph_timing: device events around 20 launches, each with its weight upload), `--repeats`
                  times: min / median / max, and the bytes the layout says one launch moves (32 in, 32 out and 4 of row length a vertex, 8 a
                  slice, 32 an entry that is not padding, 4 a target) over the median.
  k_skin          THE YARDSTICK: the parent's streaming kernel over the same vertex format, on a skin of `--bones` bones over the same
                  vertices, timed the same way in the same run (glz_debug_skin_timing), 88 bytes a vertex; its spread between repeats is
                  what a difference has to exceed to mean anything.
  k_morph_skin    the fused kernel on the 8 dense targets attached to that skin, against k_morph (from the skin's bind pose) plus k_skin
                  timed separately; and k_morph_skin_dq, the same with the skin set to dual-quaternion mode, turn by turn with it.
  animate         median wall time around animate() of the free-standing morph, against update_vertices() fed the vertices glz_host_morph
                  made of the same weights BEFORE the clock starts, alternating call by call; and the update_ms of both.

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


def make_targets(rng, n, kind):
    if kind == "8 dense":
        return [(None, (rng.normal(size=(n, 3)) * 1e-3).astype(np.float32), (rng.normal(size=(n, 3)) * 1e-2).astype(np.float32)) for _ in range(8)]
    out = []
    for _ in range(50):
        idx = np.nonzero(rng.random(n) < 0.1)[0].astype(np.uint32)
        out.append((idx, (rng.normal(size=(len(idx), 3)) * 1e-3).astype(np.float32), (rng.normal(size=(len(idx), 3)) * 1e-2).astype(np.float32)))
    return out


def spread(values):
    return {"min": min(values), "median": statistics.median(values), "max": max(values)}


def measure(emit, inst, name, desc, kinds, args):
    inst.set_as_levels("flat")
    try:
        scene = glaze_amd.RayTraceScene.from_desc(inst, desc)
    finally:
        inst.set_as_levels("auto")
    r = glaze_amd.RayTraceRenderer.new(inst, scene, 64, 64)
    base = np.ascontiguousarray(desc.vertices).view(np.float32).reshape(-1, 8)
    n = base.shape[0]
    rng = np.random.default_rng(1)
    rows = []
    kept = {}
    for kind in kinds:
        targets = make_targets(rng, n, kind)
        kept[kind] = targets
        weights = [rng.normal(size=len(targets)).astype(np.float32) for _ in range(2)]
        t0 = time.perf_counter()
        made = [glaze_amd.host_morph(base, targets, w) for w in weights]
        host_ms = (time.perf_counter() - t0) * 1e3 / len(weights)
        morph = r.add_morph(0, targets, n_vertices=n)
        timed = [r.debug_morph_timing({morph: weights[0]}, reps=20) for _ in range(args.repeats)]
        ms, nbytes = spread([t[0] for t in timed]), timed[0][1]
        r.update_vertices(made[1], first=0)                                                       # the first refit makes the plan: not timed
        r.animate(morphs={morph: weights[0]})
        wall = {"animate": [], "update": []}
        stream = {"animate": [], "update": []}
        for i in range(2 * args.reps):
            k = (i // 2) % 2
            which = "animate" if i % 2 == 0 else "update"
            t0 = time.perf_counter()
            if which == "animate":
                r.animate(morphs={morph: weights[k]})
            else:
                r.update_vertices(made[1 - k], first=0)
            wall[which].append((time.perf_counter() - t0) * 1e3)
            stream[which].append(float(scene.info().build_ms))                                    # = glz_geometry_update_info::update_ms
        r.animate(morphs={morph: weights[0]})
        same = bool(np.array_equal(r.read_vertices(0, n).view(np.uint32), made[0].view(np.uint32)))
        r.remove_morph(morph)
        r.update_vertices(base, first=0)
        row = {"scene": name, "what": "k_morph, " + kind, "vertices": n, "entries": int((nbytes - n * 68 - ((n + 63) // 64) * 8 - 4 * len(targets)) // 32), "k_morph_ms": ms,
               "k_morph_bytes": nbytes, "k_morph_TB_per_s": nbytes / (ms["median"] * 1e-3) / 1e12, "animate_wall_ms": spread(wall["animate"]),
               "animate_update_ms": statistics.median(stream["animate"]), "update_vertices_wall_ms": spread(wall["update"]),
               "update_vertices_update_ms": statistics.median(stream["update"]), "host_morph_ms": host_ms, "animated_equals_host_morph": same}
        row["wall_ratio"] = row["animate_wall_ms"]["median"] / row["update_vertices_wall_ms"]["median"]
        emit(json.dumps(row))
        rows.append(row)
    # the yardstick and the fused kernel: a skin over every vertex, the 8 dense targets attached to it
    joints, sw, axis, centre = chain(desc.vertices, args.bones)
    bones = twist(args.bones, axis, centre, 0.05)
    skin = r.add_skin(0, joints, sw, args.bones)
    targets = kept["8 dense"]
    w = rng.normal(size=len(targets)).astype(np.float32)
    morph = r.add_morph(0, targets, skin=skin)
    skin_ms, morph_ms, fused_ms, fused_dq_ms = [], [], [], []
    fused_bytes = fused_dq_bytes = 0
    for _ in range(args.repeats):                                                                 # the four take turns
        skin_ms.append(r.debug_skin_timing(skin, bones, reps=20))
        morph_ms.append(r.debug_morph_timing({morph: w}, reps=20)[0])
        t, fused_bytes = r.debug_morph_timing({morph: w}, {skin: bones}, reps=20)
        fused_ms.append(t)
        r.set_skin_blend(skin, "dual_quaternion")                                                 # the same skin in the other mode: k_morph_skin_dq
        t, fused_dq_bytes = r.debug_morph_timing({morph: w}, {skin: bones}, reps=20)
        fused_dq_ms.append(t)
        r.set_skin_blend(skin, "linear")
    r.set_skin_blend(skin, "dual_quaternion")
    r.animate(morphs={morph: w}, poses={skin: bones})
    want = glaze_amd.host_skin(glaze_amd.host_morph(base, targets, w), joints, sw, bones, blend="dual_quaternion")
    same_dq = bool(np.array_equal(r.read_vertices(0, n).view(np.uint32), want.view(np.uint32)))
    r.set_skin_blend(skin, "linear")
    r.animate(morphs={morph: w}, poses={skin: bones})
    want = glaze_amd.host_skin(glaze_amd.host_morph(base, targets, w), joints, sw, bones)
    same = bool(np.array_equal(r.read_vertices(0, n).view(np.uint32), want.view(np.uint32)))
    ks, km, kf = spread(skin_ms), spread(morph_ms), spread(fused_ms)
    yard = {"scene": name, "what": "k_skin, the yardstick", "vertices": n, "bones": args.bones, "k_skin_ms": ks, "k_skin_bytes": SKIN_BYTES_PER_VERTEX * n,
            "k_skin_TB_per_s": SKIN_BYTES_PER_VERTEX * n / (ks["median"] * 1e-3) / 1e12,
            "k_skin_TB_per_s_spread": [SKIN_BYTES_PER_VERTEX * n / (ks[k] * 1e-3) / 1e12 for k in ("max", "min")]}
    fused = {"scene": name, "what": "k_morph_skin, 8 dense", "k_morph_skin_ms": kf, "k_morph_ms": km, "k_skin_ms": ks, "k_morph_skin_bytes": fused_bytes,
             "k_morph_skin_TB_per_s": fused_bytes / (kf["median"] * 1e-3) / 1e12, "fused_over_separate": kf["median"] / (km["median"] + ks["median"]),
             "animated_equals_host_skin_of_host_morph": same}
    kd = spread(fused_dq_ms)
    fused_dq = {"scene": name, "what": "k_morph_skin_dq, 8 dense", "k_morph_skin_dq_ms": kd, "k_morph_skin_dq_bytes": fused_dq_bytes,
                "k_morph_skin_dq_TB_per_s": fused_dq_bytes / (kd["median"] * 1e-3) / 1e12, "dq_over_linear": kd["median"] / kf["median"],
                "animated_equals_host_skin_dq_of_host_morph": same_dq}
    emit(json.dumps(yard))
    emit(json.dumps(fused))
    emit(json.dumps(fused_dq))
    emit("")
    emit("%s, %d vertices" % (name, n))
    emit("")
    emit("| kernel | ms, min / median / max | bytes a launch | TB/s at the median |")
    emit("|---|---|---|---|")
    for row in rows:
        emit("| %s | %.4f / %.4f / %.4f | %d | %.2f |" % (row["what"], row["k_morph_ms"]["min"], row["k_morph_ms"]["median"], row["k_morph_ms"]["max"], row["k_morph_bytes"],
                                                          row["k_morph_TB_per_s"]))
    emit("| k_skin (yardstick) | %.4f / %.4f / %.4f | %d | %.2f (%.2f .. %.2f) |" % (ks["min"], ks["median"], ks["max"], yard["k_skin_bytes"], yard["k_skin_TB_per_s"],
                                                                                     *yard["k_skin_TB_per_s_spread"]))
    emit("| k_morph_skin, 8 dense | %.4f / %.4f / %.4f | %d | %.2f |" % (kf["min"], kf["median"], kf["max"], fused_bytes, fused["k_morph_skin_TB_per_s"]))
    emit("| k_morph_skin_dq, 8 dense (against k_morph_skin %.2f) | %.4f / %.4f / %.4f | %d | %.2f |" % (fused_dq["dq_over_linear"], kd["min"], kd["median"], kd["max"],
                                                                                                     fused_dq_bytes, fused_dq["k_morph_skin_dq_TB_per_s"]))
    emit("| k_morph from the bind pose + k_skin, separately | %.4f + %.4f = %.4f (fused / separate %.2f) | | |" % (km["median"], ks["median"], km["median"] + ks["median"],
                                                                                                                fused["fused_over_separate"]))
    emit("")
    emit("| targets | animate: wall (ms) | update_ms | update_vertices: wall (ms) | update_ms | animate / update_vertices (wall) | host blending, in neither (ms) | bits equal |")
    emit("|---|---|---|---|---|---|---|---|")
    for row in rows:
        emit("| %s | %.3f | %.3f | %.3f | %.3f | %.2f | %.1f | %s |" % (row["what"][9:], row["animate_wall_ms"]["median"], row["animate_update_ms"],
                                                                        row["update_vertices_wall_ms"]["median"], row["update_vertices_update_ms"], row["wall_ratio"],
                                                                        row["host_morph_ms"], "yes" if row["animated_equals_host_morph"] else "NO"))
    emit("")
    del r, scene


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", nargs="+", default=["small", "large"])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--bones", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "morph_timing.txt"))
    args = ap.parse_args()
    lines = []

    def emit(text):
        print(text, flush=True)
        lines.append(text)

    inst = glaze_amd.RayTraceInstance.new()
    if "small" in args.scenes:
        measure(emit, inst, "atrium 262 k", atrium_scene(texture_size=256, sky_size=(512, 256)), ("8 dense", "50 sparse"), args)
    if "large" in args.scenes:
        measure(emit, inst, "atrium 7.2 M", atrium_scene(detail=16.0, texture_size=256, sky_size=(512, 256)), ("8 dense",), args)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
