"""What playing clips on the device costs (RayTraceRenderer.play) against what there was before: the clip evaluated on the host
(glaze_amd.host_clip_bones, per character) and pose() fed the bones -- the same scene, the same skins, the same times, the same process.

    python tools/gpu_clip_timing.py [--configs one crowd chain] [--reps 9] [--kernel-repeats 7]

The scene is the atrium at its small detail (flattened); skins take consecutive vertex ranges of it, 1/256 of the vertices each.
  one    one skin of 64 bones, a random tree;
  crowd  256 skins of 64 bones each, every skeleton a two-level forest (8 roots with 7 children each), all 256 played in one call;
  chain  one skin whose skeleton is one chain 1 024 bones deep: 1 024 levels of one bone, the worst case of k_clip_bones' level loop.
Clips have 8 keys with translation, rotation and scale tracks, small motions; two times between keys alternate.  Per configuration:

  k_clip_bones    the kernel alone, one launch for all the plays (glz_debug_clip_timing: device events around 20 launches),
                  --kernel-repeats measurements: the median and the lowest and highest;
  play            wall time around play(): the table of plays up, k_clip_bones, k_skin per skin, derivatives, refit; and its update_ms;
  host + pose     wall time around host_clip_bones for every skin and then pose() with the bones it made; the host's evaluation alone
                  is given too (it is part of this figure), and pose()'s update_ms.

play and host + pose alternate call by call, --reps of each, so that what else the host does falls on both; medians and ranges.  After
the timed calls the vertices play leaves are compared with those pose leaves, bit for bit.  One JSON line per configuration, then a
markdown table.  No threshold is held: the yardstick, pose, is measured in the same run.
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

F = np.float32


def skeleton(kind, rng):
    if kind == "chain":
        return np.arange(-1, 1023, dtype=np.int32)
    if kind == "crowd":                                                                           # 8 roots, then 7 children of each
        return np.concatenate([np.full(8, -1), np.repeat(np.arange(8), 7)]).astype(np.int32)
    p = np.full(64, -1, np.int32)
    for b in range(1, 64):
        p[b] = rng.integers(0, b)
    return p


def levels(parents):
    depth = []
    for p in parents:
        depth.append(0 if p < 0 else depth[p] + 1)
    return max(depth) + 1


def clip(rng, n_bones, n_keys, reach, turn):
    times = np.arange(n_keys, dtype=F)
    tr = rng.uniform(-reach, reach, (n_keys, n_bones, 3)).astype(F)
    ro = np.concatenate([rng.normal(0, turn, (n_keys, n_bones, 3)), np.ones((n_keys, n_bones, 1))], -1).astype(F)
    sc = rng.uniform(0.999, 1.001, (n_keys, n_bones, 3)).astype(F)
    return times, tr, ro, sc


def spread(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["one", "crowd", "chain"])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--kernel-repeats", type=int, default=7)
    args = ap.parse_args()
    inst = glaze_amd.RayTraceInstance.new()
    desc = atrium_scene(texture_size=256, sky_size=(512, 256))
    per_skin = desc.vertices.shape[0] // 256
    rows = []
    for kind in args.configs:
        rng = np.random.default_rng(5)
        inst.set_as_levels("flat")
        try:
            scene = glaze_amd.RayTraceScene.from_desc(inst, desc)
        finally:
            inst.set_as_levels("auto")
        r = glaze_amd.RayTraceRenderer.new(inst, scene, 64, 64)
        n_skins = 256 if kind == "crowd" else 1
        chars = []
        for s in range(n_skins):
            parents = skeleton(kind, rng)
            k = len(parents)
            joints = rng.integers(0, k, (per_skin, 4)).astype(np.uint16)
            w = rng.uniform(0.1, 1.0, (per_skin, 4))
            skin = r.add_skin(s * per_skin, joints, (w / w.sum(1, keepdims=True)).astype(F), k)
            ib = np.tile(np.eye(4, dtype=F).reshape(16), (k, 1))
            keys = clip(rng, k, 8, 1e-2 / k, 1e-2 / k)
            sk = r.add_skeleton(skin, parents, ib)
            chars.append({"skin": skin, "parents": parents, "ib": ib, "keys": keys, "clip": r.add_clip(sk, *keys)})
        times = (2.25, 5.5)

        def plays(t):
            return [(c["clip"], t) for c in chars]

        def host_bones(t):
            return {c["skin"]: glaze_amd.host_clip_bones(c["parents"], c["ib"], c["keys"][0], c["keys"][1], c["keys"][2], t, scales=c["keys"][3]) for c in chars}

        r.play(plays(times[0]))                                                                   # the first refit makes the plan: not timed
        r.pose(host_bones(times[1]))
        wall = {"play": [], "pose": [], "host": []}
        stream = {"play": [], "pose": []}
        for i in range(2 * args.reps):
            t = times[(i // 2) % 2]
            t0 = time.perf_counter()
            if i % 2 == 0:
                r.play(plays(t))
            else:
                bones = host_bones(t)
                t1 = time.perf_counter()
                r.pose(bones)
                wall["host"].append((t1 - t0) * 1e3)
            which = "play" if i % 2 == 0 else "pose"
            wall[which].append((time.perf_counter() - t0) * 1e3)
            stream[which].append(float(scene.info().build_ms))                                    # = glz_geometry_update_info::update_ms
        n_all = n_skins * per_skin
        r.play(plays(times[0]))
        played = r.read_vertices(0, n_all)
        r.pose(host_bones(times[0]))
        same = bool(np.array_equal(played.view(np.uint32), r.read_vertices(0, n_all).view(np.uint32)))
        kernel = [r.debug_clip_timing(plays(times[i % 2]), reps=20) for i in range(args.kernel_repeats)]
        row = {"config": kind, "skins": n_skins, "bones_per_skin": len(chars[0]["parents"]), "levels": levels(chars[0]["parents"]),
               "vertices_per_skin": per_skin, "k_clip_bones_ms": spread(kernel), "play_wall_ms": spread(wall["play"]), "play_update_ms": spread(stream["play"]),
               "host_and_pose_wall_ms": spread(wall["pose"]), "host_clip_bones_ms": spread(wall["host"]), "pose_update_ms": spread(stream["pose"]),
               "play_over_host_and_pose": statistics.median(wall["play"]) / statistics.median(wall["pose"]), "play_equals_pose_bit_for_bit": same}
        print(json.dumps(row), flush=True)
        rows.append(row)
        del r, scene
    print("| configuration | skins x bones | levels | k_clip_bones alone (ms, median) | min - max | play: wall (ms) | min - max | update_ms | host_clip_bones + pose: wall (ms) | min - max | of it host_clip_bones (ms) | pose's update_ms | play / (host + pose) | bits equal |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for w in rows:
        k, p, q, h = w["k_clip_bones_ms"], w["play_wall_ms"], w["host_and_pose_wall_ms"], w["host_clip_bones_ms"]
        print("| %s | %d x %d | %d | %.4f | %.4f - %.4f | %.3f | %.3f - %.3f | %.3f | %.3f | %.3f - %.3f | %.3f | %.3f | %.2f | %s |" % (
            w["config"], w["skins"], w["bones_per_skin"], w["levels"], k["median"], k["min"], k["max"], p["median"], p["min"], p["max"], w["play_update_ms"]["median"], q["median"], q["min"],
            q["max"], h["median"], w["pose_update_ms"]["median"], w["play_over_host_and_pose"], "yes" if w["play_equals_pose_bit_for_bit"] else "NO"))


if __name__ == "__main__":
    main()
