"""Two builds of the library side by side: python tools/gpu_compare_builds.py variants/libglaze_hip_OLD.so [launches]

  structures  what a scene build leaves behind, bit for bit: debug_bvh() (nodes, triangles), debug_bvh8(), debug_tlas_instances() and every
              field of info() but build_ms and bvh_sah_cost (a float atomic sums those two in no fixed order) -- mattest.glaze under every
              builder, the atrium, the atrium at 7.2 M triangles (many levels of several blocks per node), a two-level forest, tiny cubes
  build times info().build_ms of seven builds after one discarded first build, per row but the tiny ones: median, minimum, maximum per
              library, and whether the new median stays within the old median plus the old build's own range
  renders     the same renders (a NaN's sign and payload are not part of the contract, every NaN is made the same one)

Each build of the library works in child processes of its own, one per part, run alternately (new, old, new, old, ...) so that both see
the same neighbours on the machine; every child has a time limit, and the first one that fails ends the run."""
import os
import subprocess
import sys
import tempfile

import numpy as np

code = r'''
import json, os, sys
sys.path.insert(0, ".")
import numpy as np
import glaze_amd
from glaze_amd.scenes import atrium_scene, cube_scene, forest_scene
part, out, launches = sys.argv[1], sys.argv[2], int(sys.argv[3])
res = {}

def build_row(name, make, builder="auto", levels="auto", timed=True):
    """structures of a first build, then build_ms of seven more"""
    inst = glaze_amd.RayTraceInstance.new()
    inst.set_bvh_builder(builder)
    inst.set_as_levels(levels)
    scene = make(inst)
    i = scene.info()
    res[name + "/nodes"], res[name + "/tris"] = scene.debug_bvh()
    res[name + "/nodes8"] = scene.debug_bvh8()
    res[name + "/tlas"] = scene.debug_tlas_instances()
    res[name + "/info"] = np.array(json.dumps({f: (list(getattr(i, f)) if hasattr(getattr(i, f), "__len__") else getattr(i, f))
                                               for f, _ in i._fields_ if f not in ("build_ms", "bvh_sah_cost")}))
    del scene
    if timed:
        ms = []
        for _ in range(7):
            scene = make(inst)
            ms.append(scene.info().build_ms)
            del scene
        res[name + "/build_ms"] = np.array(ms, np.float64)

if part == "structures":
    mattest = os.path.join("tests", "golden", "mattest.glaze")
    for b in ("lbvh", "ploc", "sah", "sah_host"):
        build_row("mattest " + b, lambda inst: glaze_amd.RayTraceScene.new(inst, glaze_amd.parse(mattest)), builder=b)   # (a scene consumes what was parsed)
    desc = atrium_scene()
    build_row("atrium", lambda inst: glaze_amd.RayTraceScene.from_desc(inst, desc))
    desc = forest_scene(200)
    build_row("forest 200, two levels", lambda inst: glaze_amd.RayTraceScene.from_desc(inst, desc), levels="two_level")
    for ntri in (1, 2, 3, 5, 12):
        desc = cube_scene()
        desc.indices = desc.indices[: 3 * ntri].copy()
        desc.meshes["index_count"][0] = 3 * ntri
        build_row("cube, %d triangles" % ntri, lambda inst: glaze_amd.RayTraceScene.from_desc(inst, desc), timed=False)
elif part == "structures, 7.2 M triangles":
    desc = atrium_scene(detail=16.0, texture_size=256)
    build_row("atrium 7.2 M", lambda inst: glaze_amd.RayTraceScene.from_desc(inst, desc))
else:
    inst = glaze_amd.RayTraceInstance.new()
    for name, like in (("atrium", False), ("sponza_like", True)):
        scene = glaze_amd.RayTraceScene.from_desc(inst, atrium_scene(sponza_like=like))
        r = glaze_amd.RayTraceRenderer.new(inst, scene, 1920, 1080)
        r.set_depth(8); r.set_seed(5)
        for chains in (1, 3):
            r.set_chains(chains); r.restart(); r.step(launches); r.wait_idle()
            res["%s_chains%d_hdr" % (name, chains)] = r.read_hdr()
            res["%s_chains%d_out" % (name, chains)] = r.read_result()
np.savez(out, **res)
'''
old = os.path.abspath(sys.argv[1])
launches = sys.argv[2] if len(sys.argv) > 2 else "128"
tmp = tempfile.mkdtemp()
# part -> time limit of one child in seconds: tens of builds that take milliseconds on the device and up to a second on the host; eight
# scenes of 7.2 M triangles; four renders of `launches` launches at 1920 x 1080
parts = {"structures": 300, "structures, 7.2 M triangles": 300, "renders": 600}
results = {"new": {}, "old": {}}
for n_part, (part, limit) in enumerate(parts.items()):
    for tag, lib in (("new", None), ("old", old)):
        env = dict(os.environ)
        if lib:
            env["GLAZE_HIP_LIB"] = lib
        path = os.path.join(tmp, "%s%d.npz" % (tag, n_part))
        print("-- %s, %s build" % (part, tag), flush=True)
        subprocess.run([sys.executable, "-c", code, part, path, launches], env=env, check=True, timeout=limit)
        results[tag].update(np.load(path))
a, b = results["new"], results["old"]
bad = 0
if sorted(a) != sorted(b):
    print("the two builds gave different sets of results: %s" % sorted(set(a) ^ set(b)))
    bad += 1
print("structures")
for k in a:
    if "/" not in k or k.endswith("/build_ms") or k not in b:
        continue
    same = a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes()
    bad += not same
    print("  %-40s %-12s %s" % (k, "x".join(map(str, a[k].shape)) or "-", "identical" if same else "DIFFERENT"))
print("build times (info().build_ms, seven builds after a discarded first): median [minimum .. maximum] ms")
slower = 0
for k in a:
    if not k.endswith("/build_ms") or k not in b:
        continue
    (nm, nlo, nhi), (om, olo, ohi) = ((float(np.median(x[k])), float(x[k].min()), float(x[k].max())) for x in (a, b))
    within = nm <= om + (ohi - olo)
    slower += not within
    print("  %-28s new %8.3f [%8.3f .. %8.3f]   old %8.3f [%8.3f .. %8.3f]   new median %s old median + old range (%.3f)" % (
        k[:-len("/build_ms")], nm, nlo, nhi, om, olo, ohi, "<=" if within else "ABOVE", om + (ohi - olo)))
print("renders")
for k in a:
    if "/" in k or k not in b:
        continue
    x, y = np.nan_to_num(a[k], nan=-1.0).view(np.uint32), np.nan_to_num(b[k], nan=-1.0).view(np.uint32)
    raw = int((a[k].view(np.uint32) != b[k].view(np.uint32)).any(-1).sum())
    d = int((x != y).any(-1).sum())
    bad += d
    print("  %-28s pixels that differ: %d (raw words, NaN payloads included: %d; NaN pixels %d / %d)" % (k, d, raw, int(np.isnan(a[k]).any(-1).sum()), int(np.isnan(b[k]).any(-1).sum())))
print("identical" if bad == 0 else "DIFFERENT")
if slower:
    print("%d build-time rows above the old build's median + range" % slower)
sys.exit(1 if bad or slower else 0)
