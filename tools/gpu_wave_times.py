"""When the waves of one k_trace finish (variant built with -DGLZ_WAVE_TIMES): share of the frame WORLD, one chain.
SCENE=atrium (1920 x 1080, the bench workload) or mattest (tests/golden/mattest.glaze at 1024 x 1024), depth 8.  With LAUNCHES=2 the kernel
looked at also traces the shadow rays of the launch before, and where its waves specialise the two kinds are told apart -- a shadow wave
has no closest-hit pass, its second stamp follows its first within the kernel's prologue -- and listed each on its own: when the first, the median and the last
wave of the kind end, as fractions of the kernel's duration, and the wave-slot time left idle between a wave's end and the kernel's."""
import ctypes, os, sys
import numpy as np
sys.path.insert(0, ".")
import glaze_amd
from glaze_amd.scenes import atrium_scene
lib = ctypes.CDLL(os.environ["GLAZE_HIP_LIB"])
inst = glaze_amd.RayTraceInstance.new()
if os.environ.get("SCENE", "atrium") == "mattest":
    scene = glaze_amd.RayTraceScene.new(inst, glaze_amd.parse(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "mattest.glaze")))
    r = glaze_amd.RayTraceRenderer.new(inst, scene, 1024, 1024)
else:
    scene = glaze_amd.RayTraceScene.from_desc(inst, atrium_scene())
    r = glaze_amd.RayTraceRenderer.new(inst, scene, 1920, 1080)
r.set_depth(8)
r.enable_counters(False, False)
for world in [int(w) for w in os.environ.get("WORLDS", "8,1").split(",")]:
    r.set_partition(0, world)
    r.set_chains(1)
    r.restart(); r.step(24); r.wait_idle()
    for rep in range(3):
        r.step(int(os.environ.get("LAUNCHES", "1"))); r.wait_idle()   # LAUNCHES=2: the last k_trace also traces the shadow rays of the launch before
        t = np.zeros(3 * 8192, dtype=np.uint64)
        assert lib.glz_debug_wave_times(t.ctypes.data_as(ctypes.c_void_p), 8192) == 0
        t = t.reshape(-1, 3).astype(np.int64)
        t = t[t[:, 0] > 0]
        t0 = t[:, 0].min()
        us = (t - t0) / 100.0   # wall_clock64: 100 MHz
        end = np.sort(us[:, 2])
        print("world %d rep %d: %d waves, start spread %.1f us, closest done p50/p90/p99/max %.1f/%.1f/%.1f/%.1f us, end p10/p50/p75/p90/p95/p99/max %.1f/%.1f/%.1f/%.1f/%.1f/%.1f/%.1f us" % (
            world, rep, len(t), us[:, 0].max(), *np.percentile(us[:, 1], [50, 90, 99, 100]), *np.percentile(end, [10, 50, 75, 90, 95, 99, 100])), flush=True)
        # the two kinds of wave of a kernel whose waves specialise (kernels_render.hip k_trace): ends as fractions of the kernel, idle wave-slot time
        length = us[:, 2].max()
        shadow = (us[:, 1] - us[:, 0]) < 20.0   # the prologue (staged tree top, the plan) takes a few us, a closest-hit pass of several groups hundreds
        if shadow.any() and not shadow.all():
            idle = length - us[:, 2]
            for name, sel in (("closest-hit", ~shadow), ("shadow", shadow)):
                e = us[sel, 2] / length
                print("   %-11s %5d waves: first / median / last end at %.3f / %.3f / %.3f of the kernel's %.1f us; idle after their ends %.2f %% of all wave-slot time" % (
                    name, int(sel.sum()), e.min(), np.median(e), e.max(), length, 100.0 * idle[sel].sum() / (length * len(us))), flush=True)
            print("   idle wave-slot time between a wave's end and the kernel's: %.2f %% of all" % (100.0 * idle.sum() / (length * len(us))), flush=True)
        # what sharing work inside a block (4 consecutive waves) could reach at best: the slowest block's mean against the slowest wave
        work = (us[:, 2] - us[:, 0])
        nb = len(work) // 4
        blk = work[:nb * 4].reshape(nb, 4)
        print("   slowest wave %.1f us; slowest block mean %.1f us (its waves %s); blocks of 8 waves: %.1f us" % (
            work.max(), blk.mean(axis=1).max(), np.round(blk[blk.mean(axis=1).argmax()], 1), work[:(len(work) // 8) * 8].reshape(-1, 8).mean(axis=1).max()), flush=True)
        st = np.zeros(8 * 8192, dtype=np.uint32)
        if hasattr(lib, "glz_debug_wave_stats") and lib.glz_debug_wave_stats(st.ctypes.data_as(ctypes.c_void_p), 8192) == 0:
            st = st.reshape(-1, 8).astype(np.float64)[: len(us)]
            dur = us[:, 1] - us[:, 0]
            busy = dur > 5.0
            order = np.argsort(dur)
            def row(name, sel):
                x = st[sel]
                print("   %-14s %5d waves: %.1f us, rounds %.0f, node iterations %.0f with %.1f lanes, leaf iterations %.0f with %.1f lanes, rounds with helpers %.0f, rounds only waiting for helpers %.0f, us per node iteration %.3f" % (
                    name, len(x), dur[sel].mean(), x[:, 0].mean(), x[:, 1].mean(), x[:, 2].sum() / max(x[:, 1].sum(), 1), x[:, 3].mean(), x[:, 4].sum() / max(x[:, 3].sum(), 1),
                    x[:, 5].mean(), x[:, 6].mean(), dur[sel].sum() / max(x[:, 1].sum(), 1)), flush=True)
            nb = int(busy.sum())
            ob = order[-nb:]
            row("all", ob)
            row("fastest tenth", ob[: nb // 10])
            row("median tenth", ob[nb // 2 - nb // 20: nb // 2 + nb // 20])
            row("slowest tenth", ob[-(nb // 10):])
            row("slowest 1 %", ob[-max(nb // 100, 1):])
        # where the slow waves are: by XCD (consecutive blocks go to consecutive XCDs) and by position in the grid (= in the image: wave w
        # traces the groups w, w + n_waves, ...)
        dur = us[:, 1] - us[:, 0]
        blk_id = np.arange(len(dur)) // 4
        print("   closest phase by XCD (block %% 8): %s us" % " ".join("%.0f" % dur[blk_id % 8 == x].mean() for x in range(8)), flush=True)
        print("   closest phase by sixteenth of the grid: %s us" % " ".join("%.0f" % c.mean() for c in np.array_split(dur, 16)), flush=True)
        # waves still running as a function of time
        grid = np.linspace(0, end[-1], 11)
        print("   running at", " ".join("%.0fus:%d" % (g, int(((us[:, 0] <= g) & (us[:, 2] > g)).sum())) for g in grid), flush=True)
