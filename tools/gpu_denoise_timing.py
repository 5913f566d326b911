"""Cost of the post stages on the bench atrium at 1920 x 1080: device-event medians over REPS runs of the first-hit pass (trace and
attribute kernels), the demodulation and each a-trous pass (glz_debug_post_timing), next to one render launch of the same build in the
same process and to a pass's byte floor (32 bytes read + 16 written per pixel at the 6.3 TB/s the microarchitecture notes give as
achievable), and k_despeckle alone at radius 1 and 2 on the same frame (glz_debug_despeckle's device events; same byte floor).  The render launch's total is a host clock around 64 launches that end in wait_idle; its k_trace / k_shade split is the
renderer's own device-event statistics.  Then the guide modes: the first-hit pass with the attribute kernel (first_hit) against the
chain of through_specular at caps 1 .. 8 on the atrium, which has no specular material -- every list is empty, so the slope over the cap
is the cost of two empty launches -- and on tests/golden/mattest.glaze at 1024 x 1024, where half the frame is Glass: the time every
bounce adds next to the number of rays alive in it.  Last, k_motion and k_reproject alone (glz_debug_motion_timing, glz_debug_reproject's
device events) for a camera that moved about 0.6 m and turned, next to their byte floors, and k_motion_deform (the same hook with previous
vertices) next to k_motion and to its own floor.  Run from the repository root on the GPU; writes nothing but its output."""
import os
import statistics
import sys
import time

sys.path.insert(0, ".")
import glaze_amd
from glaze_amd.scenes import atrium_scene

W, H, REPS = 1920, 1080, 64
FLOOR_US = W * H * 48 / 6.3e12 * 1e6

inst = glaze_amd.RayTraceInstance.new()
if inst is None:
    raise SystemExit("no gfx950 device")
r = glaze_amd.RayTraceRenderer.new(inst, glaze_amd.RayTraceScene.from_desc(inst, atrium_scene()), W, H)
r.set_depth(8)
r.step(24)
r.wait_idle()
s0 = r.stats()
t = time.time()
r.step(64)
r.wait_idle()
launch_ms = (time.time() - t) / 64 * 1e3
s1 = r.stats()
print("render launch: %.3f ms (k_trace %.3f, k_shade %.3f)" % (launch_ms, (s1.trace_closest_ms - s0.trace_closest_ms) / 64, (s1.shade_ms - s0.shade_ms) / 64))
for _ in range(8):
    r.debug_post_timing()                     # warm-up: code objects, first-use allocations
runs = [r.debug_post_timing() for _ in range(REPS)]


def med(f):
    return statistics.median(f(x) for x in runs) * 1e3


trace, attr, demod = med(lambda x: x["first_hit_trace"]), med(lambda x: x["first_hit_attributes"]), med(lambda x: x["demodulate"])
print("first-hit pass: trace %.1f us + attributes %.1f us = %.1f us (%.1f %% of a render launch)" % (trace, attr, trace + attr, (trace + attr) / launch_ms / 10))
print("demodulation: %.1f us" % demod)
passes = [med(lambda x, k=k: x["passes"][k]) for k in range(5)]
for k, p in enumerate(passes):
    print("a-trous pass %d (stride %2d): %.1f us = %.1f x the %.1f us byte floor" % (k, 1 << k, p, p / FLOOR_US, FLOOR_US))
print("five passes: %.1f us (floor %.1f us); with the demodulation %.1f us" % (sum(passes), 5 * FLOOR_US, sum(passes) + demod))
# ---- firefly rejection: k_despeckle alone between device events (glz_debug_despeckle), on this renderer's own frame and planes ----
frame, plane0, plane1 = r.read_result(), r.read_aov(0), r.read_aov(1)
for radius in (1, 2):
    for _ in range(4):
        inst.debug_despeckle(frame, plane0, plane1, want_ms=True, radius=radius)
    remod = statistics.median(inst.debug_despeckle(frame, plane0, plane1, want_ms=True, radius=radius)[1] for _ in range(REPS)) * 1e3
    ahead = statistics.median(inst.debug_despeckle(frame, plane0, plane1, want_ms=True, with_filter=True, radius=radius)[1] for _ in range(REPS)) * 1e3
    # the floor is the kernel's ahead of the filter (i_0 and aov0 read, one frame written); the re-modulating one reads aov1 too: 48 B + 16 B
    print("despeckle radius %d (%2d neighbours): %.1f us ahead of the filter = %.1f x the %.1f us byte floor, %.2f x a-trous pass 0; "
          "%.1f us with the re-modulating store (which also reads the albedo plane: floor %.1f us)" % (
              radius, (2 * radius + 1) ** 2 - 1, ahead, ahead / FLOOR_US, FLOOR_US, ahead / passes[0], remod, FLOOR_US * 64 / 48))
t = time.time()
for _ in range(16):
    r.read_denoised()
print("read_denoised() end to end, frame read back included: %.2f ms" % ((time.time() - t) / 16 * 1e3))
r.set_despeckle(True)
t = time.time()
for _ in range(16):
    r.read_denoised()
print("read_denoised() with the rejection enabled: %.2f ms" % ((time.time() - t) / 16 * 1e3))
t = time.time()
for _ in range(16):
    r.read_despeckled()
print("read_despeckled() end to end, frame read back included: %.2f ms" % ((time.time() - t) / 16 * 1e3))
r.set_despeckle(False)


# ---- guide modes: what follows k_first_hit (slot 'first_hit_attributes' of the timing hook) ----
def after_trace(ren, reps=REPS):
    for _ in range(4):
        ren.debug_post_timing()
    got = [ren.debug_post_timing() for _ in range(reps)]
    return statistics.median(x["first_hit_trace"] for x in got) * 1e3, statistics.median(x["first_hit_attributes"] for x in got) * 1e3


def guide_rows(name, ren, caps, counts):
    ren.set_guide_mode("first_hit")
    trace0, attr0 = after_trace(ren)
    print("%s, first_hit: trace %.1f us + attributes %.1f us = %.1f us" % (name, trace0, attr0, trace0 + attr0))
    before, rows = None, []
    for cap in caps:
        ren.set_guide_mode("through_specular", cap)
        trace, chain = after_trace(ren)
        alive = int(ren.debug_guide_chain(cap)[2].sum()) if counts else 0
        rows.append((cap, chain))
        print("%s, through_specular cap %d: trace %.1f us + chain %.1f us = %.1f us (+%.1f us on first_hit)%s" % (
            name, cap, trace, chain, trace + chain, trace + chain - trace0 - attr0,
            "" if before is None else "; bounce %d adds %.1f us%s" % (cap, chain - before, " for %d live rays" % alive if counts else "")))
        if before is None and counts:
            print("%s:   bounce 1 (in the cap-1 figure above) has %d live rays" % (name, alive))
        before = chain
    ren.set_guide_mode("first_hit")
    return attr0, rows


attr0, rows = guide_rows("atrium %d x %d" % (W, H), r, range(1, 9), False)
slope = (rows[-1][1] - rows[0][1]) / (rows[-1][0] - rows[0][0])
print("atrium: a bounce whose list is empty (k_guide_trace + k_guide_continue) costs %.1f us, one empty launch %.1f us; vertex 0 through k_guide_first "
      "%.1f us against %.1f us through k_first_hit_attributes" % (slope, slope / 2, rows[0][1] - slope, attr0))
mattest = os.path.join("tests", "golden", "mattest.glaze")
m = glaze_amd.RayTraceRenderer.new(inst, glaze_amd.RayTraceScene.new(inst, glaze_amd.parse(mattest)), 1024, 1024)
m.step(2)
m.wait_idle()
guide_rows("mattest 1024 x 1024", m, range(1, 5), True)


# ---- motion and reprojection: k_motion and k_reproject alone between device events, the atrium's camera moved and turned ----
from glaze_amd.scene_desc import _clone

desc = atrium_scene()
prev_cam = _clone(desc.camera)
prev_cam.position[:] = [a + b for a, b in zip(desc.camera.position[:], (0.45, 0.1, -0.4))]
prev_cam.target[:] = [a + b for a, b in zip(desc.camera.target[:], (0.6, -0.2, 0.5))]
motion = r.read_motion(prev_cam)
hits = float((motion[..., 2] < float("inf")).mean())
for _ in range(8):
    r.debug_motion_timing(prev_cam)
k_motion = statistics.median(r.debug_motion_timing(prev_cam) for _ in range(REPS)) * 1e3
# per pixel: hit record 16 B + instance 4 B read, 16 B written.  The four float4 of a hit's 128-byte shading record are shared by every pixel
# that shows the triangle (the atrium's walls are a few hundred pixels per triangle): at most one line per triangle of the scene moves;
# the 64 B of a transform are shared by a wave and come from cache
n_tris = r.scene.info().n_as_triangles
lo, hi = W * H * 36 / 6.3e12 * 1e6, (W * H * 36 + n_tris * 128) / 6.3e12 * 1e6
print("k_motion: %.1f us (%.1f %% of the pixels hit) = %.1f x the %.1f us floor of its per-pixel streams (36 B), %.1f x the %.1f us with every one of the "
      "scene's %d shading records read once" % (k_motion, 100 * hits, k_motion / lo, lo, k_motion / hi, hi, n_tris))
# the deforming variant (k_motion_deform): every vertex of the scene handed over as its previous one, a little displaced.  It reads no shading
# record; what it gathers instead is shared by the pixels of a triangle as the record is: the leaf's primitive word (4 B of a 48-byte BvhTri)
# and three indices (12 B) per triangle, and the caller's vertices as they were uploaded, 32 B each for the 16 B of the position
info = r.scene.info()
before = desc.vertices.copy()
before["vv"] += 0.01
for _ in range(8):
    r.debug_motion_timing(prev_cam, prev_vertices=before)
k_deform = statistics.median(r.debug_motion_timing(prev_cam, prev_vertices=before) for _ in range(REPS)) * 1e3
hi_deform = (W * H * 36 + n_tris * 16 + info.n_vertices * 32) / 6.3e12 * 1e6
print("k_motion_deform: %.1f us = %.2f x k_motion, %.1f x the %.1f us floor of the per-pixel streams (36 B), %.1f x the %.1f us with the primitive word and the indices of "
      "every triangle and every one of the %d uploaded 32-byte vertices read once" % (k_deform, k_deform / k_motion, k_deform / lo, lo, k_deform / hi_deform, hi_deform,
                                                                                     info.n_vertices))
t = time.time()
for _ in range(16):
    r.read_motion(prev_cam, prev_vertices=before)
print("read_motion() with previous vertices end to end, %d vertices uploaded and the frame read back: %.2f ms" % (info.n_vertices, (time.time() - t) / 16 * 1e3))
r.update_camera(prev_cam)
prev0, prev1 = r.read_aov(0), r.read_aov(1)
r.update_camera(desc.camera)
for _ in range(4):
    inst.debug_reproject(motion, frame, prev0, prev1, want_ms=True)
out, _ = inst.debug_reproject(motion, frame, prev0, prev1, want_ms=True)
k_reproject = statistics.median(inst.debug_reproject(motion, frame, prev0, prev1, want_ms=True)[1] for _ in range(REPS)) * 1e3
floor = W * H * 80 / 6.3e12 * 1e6   # four planes read once each (a wave's taps share their lines), one written
print("k_reproject: %.1f us = %.1f x the %.1f us byte floor (80 B per pixel), %.2f x a-trous pass 0; %.1f %% of the hit pixels receive history" % (
    k_reproject, k_reproject / floor, floor, k_reproject / passes[0], 100 * float((out[..., 3] > 0).mean()) / max(hits, 1e-9)))
t = time.time()
for _ in range(16):
    r.read_motion(prev_cam)
print("read_motion() end to end, frame read back included: %.2f ms" % ((time.time() - t) / 16 * 1e3))
t = time.time()
for _ in range(16):
    r.reproject(prev_cam, frame, prev0, prev1)
print("reproject() end to end, three frames uploaded and one read back: %.2f ms" % ((time.time() - t) / 16 * 1e3))
