"""Wall-clock of ssx_spectral_import and ssx_spectral_moments_import at 512^2, 16 and 64 bins: medians over 16 alternating calls on one context, after three
warm-up pairs (one JSON line per bin count).      python tools/moments_import_cost.py"""
import ctypes as C, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from simple_spectral_amd import Options, Renderer

for bins in (16, 64):
    r = Renderer(Options(scene_name="cornell-srgb", res=(512, 512), spp=4, texture="crystal-lizard-512.png"))
    r.set_spectral_bins(bins); r.set_spectral_moments(True)
    r.render_start(); r.render_wait()
    info, sums, s2 = r.export_sums()
    sinfo, S, N = r.export_spectral()
    _, Q = r.export_moments()
    r.import_sums(info, sums)
    def t_bins():
        t = time.perf_counter(); r._check(r._lib.ssx_spectral_import(r._ctx, C.byref(sinfo), S.ctypes.data, N.ctypes.data)); return (time.perf_counter() - t) * 1e3
    def t_q():
        t = time.perf_counter(); r._check(r._lib.ssx_spectral_moments_import(r._ctx, C.byref(sinfo), Q.ctypes.data)); return (time.perf_counter() - t) * 1e3
    for _ in range(3):
        t_bins(); t_q()
    a, b = [], []
    for _ in range(16):
        a.append(t_bins()); b.append(t_q())
    ok = np.array_equal(r.export_moments()[1].view(np.uint64), Q.view(np.uint64))
    print(json.dumps({"res": 512, "bins": bins, "spectral_import_ms": round(statistics.median(a), 3), "moments_import_ms": round(statistics.median(b), 3),
                      "ratio": round(statistics.median(b) / statistics.median(a), 3), "min_max_bins": [round(min(a), 3), round(max(a), 3)],
                      "min_max_q": [round(min(b), 3), round(max(b), 3)], "round_trip_equal": bool(ok)}), flush=True)
