"""The spectral noise figure without a GPU (include/ssx.h "Spectral noise figure"): the symbols, the numpy restatement held against a second, plain per-pixel
Python loop (ragged images, thin sub-bins, masks, a NaN flux, foreign tiles), against statistics, the hosts' derivation and CSV writer, and the CLI's refusals."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import spectral_noise_ref as ref
import spectral_stats_ref as stats_ref
from simple_spectral_amd import _capi, build as sbuild
from simple_spectral_amd import renderer as rmod
from simple_spectral_amd.dist import tile_owner_mask

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "simple-spectral")
LMIN, LSTEP = np.float32(380.0), np.float32(100.0)


def bits_equal(a, b):
    """bit for bit, a NaN equal to a NaN"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype.kind != "f":
        return a.dtype == b.dtype and np.array_equal(a, b)
    nan = np.isnan(a)
    return a.dtype == b.dtype and np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint64)[~nan], b.view(np.uint64)[~nan])


def synthetic(rng, H, W, spp, bins, mean=1.0, sigma=0.5):
    """(S, Q, N) of Gaussian hero fluxes with uniform wavelengths"""
    flux = rng.normal(mean, sigma, size=(H, W, spp, 4)).astype(np.float32)
    lam = (LMIN + np.float32(0.999) * LSTEP * rng.random(size=(H, W, spp), dtype=np.float32)).astype(np.float32)
    return stats_ref.restate_sums(flux, lam, LMIN, LSTEP, bins)


def plain_loop(S, Q, N, mask=None, owner=None):
    """The definition once more, without numpy arithmetic: Python floats (binary64, IEEE) pixel by pixel, bin by bin.  Returns what ref.tile_partials and
    ref.totals return."""
    H, W, B = S.shape
    M = B // 4
    tiles_x, tiles_y = (W + 7) // 8, (H + 7) // 8
    owned = None if owner is None else tile_owner_mask(W, H, *owner)
    tEV = [[0.0] * B for _ in range(tiles_x * tiles_y)]; tEM = [[0.0] * B for _ in range(tiles_x * tiles_y)]
    tPP = [[0] * B for _ in range(tiles_x * tiles_y)]; tPU = [[0] * B for _ in range(tiles_x * tiles_y)]
    for t in range(tiles_x * tiles_y):
        ty, tx = divmod(t, tiles_x)
        if owned is not None and not owned[ty * 8, tx * 8]:
            continue
        for j in range(ty * 8, min(ty * 8 + 8, H)):
            for i in range(tx * 8, min(tx * 8 + 8, W)):
                if mask is not None and not mask[j, i]:
                    continue
                for b in range(B):
                    n = int(N[j, i, b % M])
                    if n < 2:
                        tPU[t][b] += 1
                        continue
                    s, q = float(S[j, i, b]), float(Q[j, i, b])
                    q = q - (s * s) / float(n)
                    q = 0.0 if q < 0.0 else q
                    tEV[t][b] = tEV[t][b] + (q / float(n - 1)) / float(n)
                    tEM[t][b] = tEM[t][b] + s / float(n)
                    tPP[t][b] += 1
    EV, EM, PP, PU = [0.0] * B, [0.0] * B, [0] * B, [0] * B
    for t in range(tiles_x * tiles_y):
        for b in range(B):
            EV[b] = EV[b] + tEV[t][b]; EM[b] = EM[b] + tEM[t][b]; PP[b] += tPP[t][b]; PU[b] += tPU[t][b]
    part = (np.array(tEV), np.array(tEM), np.array(tPP, dtype=np.uint32), np.array(tPU, dtype=np.uint32))
    return part, (np.array(EV), np.array(EM), np.array(PP, dtype=np.uint64), np.array(PU, dtype=np.uint64))


def both(S, Q, N, mask=None, owner=None):
    part = ref.tile_partials(S, Q, N, mask, owner)
    tot = ref.totals(*part)
    p2, t2 = plain_loop(S, Q, N, mask, owner)
    for name, a, b in zip(("tEV", "tEM", "tPP", "tPU", "EV", "EM", "PP", "PU"), part + tot, p2 + t2):
        assert bits_equal(a, b), name
    return part, tot


def test_new_symbols_exist_in_both_libraries(tmp_path):
    sbuild.build_all()
    hip, host = C.CDLL(sbuild.HIP_LIB), C.CDLL(sbuild.HOST_LIB)   # load without a GPU; no compute call is made
    for s in ("ssx_spectral_noise", "ssx_spectral_noise_reduce"):
        assert s in _capi.HIP_SYMBOLS
        getattr(hip, s)
    for s in ("ssh_spectral_noise_derive", "ssh_spectral_noise_save_csv"):
        assert s in _capi.HOST_SYMBOLS
        getattr(host, s)
    src = ('#include "ssx_host.h"\n'
           'int (*a)(ssx_ctx*, const uint8_t*, double*, double*, uint64_t*, uint64_t*, double*, double*, uint32_t*, uint32_t*) = ssx_spectral_noise;\n'
           'int (*b)(ssx_ctx*, uint32_t, uint32_t, const double*, const double*, const uint32_t*, const uint32_t*, double*, double*, uint64_t*, uint64_t*) = ssx_spectral_noise_reduce;\n'
           'int (*c)(uint32_t, const double*, const double*, const uint64_t*, const uint64_t*, double*, double*, double*) = ssh_spectral_noise_derive;\n'
           'int (*d)(const char*, uint32_t, float, float, const double*, const double*, const uint64_t*, const uint64_t*) = ssh_spectral_noise_save_csv;\n')
    open(tmp_path / "t.c", "w").write(src)
    subprocess.check_call(["gcc", "-c", "-I", os.path.join(ROOT, "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t.o")])   # the declarations are C
    from simple_spectral_amd import Renderer
    for m in ("spectral_noise", "spectral_noise_raw", "spectral_noise_reduce", "render_until_spectral"):
        assert callable(getattr(Renderer, m))
    assert callable(rmod.spectral_noise_derive)
    names = subprocess.check_output(["nm", "-D", "--defined-only", sbuild.HOST_LIB], text=True)   # the C++ host's methods
    for sym in ("_ZN3ssx8Renderer14spectral_noiseE", "_ZN3ssx8Renderer21render_until_spectralE", "_ZN3ssx21spectral_noise_deriveE"):
        assert sym in names, sym
    kernels = subprocess.check_output(["strings", sbuild.HIP_LIB], text=True)                       # the two kernels are in the library's code object
    assert "ssx_spectral_noise_tiles_kernel" in kernels and "ssx_spectral_noise_reduce_kernel" in kernels
    text = open(os.path.join(ROOT, "include", "ssx.h")).read()
    assert "e = (q / (double)(n-1)) / (double)n" in text and "noise    = sqrt(EVs / (double)P) / mean" in text and "THIS IS BIT-NEUTRAL" in text


@pytest.mark.parametrize("bins,spp", [(4, 12), (8, 24), (64, 37)])
def test_the_restatement_equals_a_plain_per_pixel_loop(bins, spp):
    """Ragged 20 x 12 (three tile columns, two rows, both edges ragged); at 64 bins and 37 spp about a third of the sub-bins are thin."""
    rng = np.random.default_rng(100 + bins)
    S, Q, N = synthetic(rng, 12, 20, spp, bins)
    thin = np.tile(N, (1, 1, 4)) < 2
    assert thin.any() == (bins == 64)
    part, tot = both(S, Q, N)
    tEV, tEM, tPP, tPU = part
    assert tEV.shape == (6, bins) and (tPP + tPU == np.array([64, 64, 32, 32, 32, 16], dtype=np.uint32)[:, None]).all()    # every in-image pixel is counted once
    assert int(tot[3].sum()) == int(thin.sum()) and int(tot[2].sum()) == int((~thin).sum())
    noise, coverage, rel = ref.derive(*tot)
    assert 0.0 < noise < 1.0 and coverage == (~thin).sum() / thin.size and rel.shape == (bins,) and np.isfinite(rel).all()
    # a mask that crosses tile boundaries and reaches the ragged edges; one pixel; nothing
    mask = np.zeros((12, 20), dtype=np.uint8); mask[5:12, 6:20] = 1; mask[2, 1] = 7
    mpart, mtot = both(S, Q, N, mask)
    assert int((mtot[2] + mtot[3])[0]) == int((mask != 0).sum())
    one = np.zeros((12, 20), dtype=np.uint8); one[9, 17] = 1
    _, otot = both(S, Q, N, one)
    e, mu, est = ref.per_pixel(S, Q, N)
    assert bits_equal(otot[0], np.where(est[9, 17], e[9, 17], 0.0)) and bits_equal(otot[1], np.where(est[9, 17], mu[9, 17], 0.0) + 0.0)
    _, ztot = both(S, Q, N, np.zeros((12, 20), dtype=np.uint8))
    znoise, zcov, zrel = ref.derive(*ztot)
    assert not ztot[0].any() and not ztot[2].any() and not ztot[3].any() and math.isnan(znoise) and math.isnan(zcov) and np.isnan(zrel).all()


def test_foreign_tiles_are_bit_neutral():
    """Two contexts (0, 2, 1) and (1, 2, 1): each one's foreign tiles hold +0.0 / 0, the merge by ownership is the whole image's partials, and each context's own
    totals -- its tiles with +0.0 added in between -- have the bits of the sum over its tiles alone."""
    rng = np.random.default_rng(5)
    S, Q, N = synthetic(rng, 12, 20, 37, 64, mean=0.25, sigma=1.0)                 # (negative means too: a partial may pass through any sign)
    whole, whole_tot = both(S, Q, N)
    owners = [(0, 2, 1), (1, 2, 1)]
    parts = []
    for owner in owners:
        part, tot = both(S, Q, N, None, owner)
        mine = tile_owner_mask(20, 12, *owner)[::8, ::8].reshape(-1)
        assert 0 < mine.sum() < 6
        for a, w in zip(part, whole):
            assert bits_equal(a[mine], w[mine]) and not a[~mine].any() and not (a.dtype.kind == "f" and np.signbit(a[~mine]).any())
        alone = ref.totals(*(a[mine] for a in part))                               # the same additions without the foreign +0.0
        for a, b in zip(tot, alone):
            assert bits_equal(a, b)
        parts.append(part)
    merged = ref.merge_owned(parts, 20, 12, owners)
    for a, w in zip(merged, whole):
        assert bits_equal(a, w)
    for a, w in zip(ref.totals(*merged), whole_tot):
        assert bits_equal(a, w)


def test_a_nan_flux_makes_the_figure_nan():
    rng = np.random.default_rng(9)
    flux = rng.normal(1.0, 0.5, size=(12, 20, 24, 4)).astype(np.float32)
    lam = (LMIN + np.float32(0.999) * LSTEP * rng.random(size=(12, 20, 24), dtype=np.float32)).astype(np.float32)
    flux[9, 17, 3, 2] = np.nan
    S, Q, N = stats_ref.restate_sums(flux, lam, LMIN, LSTEP, 8)
    assert (N >= 2).all()
    part, tot = both(S, Q, N)
    m = int(rmod.spectral_bin_index(lam[9:10, 17:18, 3:4], LMIN, LSTEP, 8)[0, 0, 0])
    b = 2 * 2 + m
    assert np.isnan(tot[0][b]) and np.isnan(tot[1][b]) and np.isnan(part[0][5, b]) and np.isfinite(np.delete(tot[0], b)).all() and np.isfinite(np.delete(part[0], 5, axis=0)).all()
    noise, coverage, rel = ref.derive(*tot)
    assert math.isnan(noise) and coverage == 1.0 and np.isnan(rel[b]) and np.isfinite(np.delete(rel, b)).all()
    assert not (noise <= 1e9)                                                         # NaN <= target is false: such a render runs to its cap
    mask = np.ones((12, 20), dtype=np.uint8); mask[9, 17] = 0                         # ... unless the mask leaves the pixel out
    assert math.isfinite(ref.figure(S, Q, N, mask)[0])


def test_the_hosts_derivation_is_the_restatements():
    rng = np.random.default_rng(11)
    S, Q, N = synthetic(rng, 12, 20, 37, 64)
    cases = [ref.totals(*ref.tile_partials(S, Q, N))]
    z = np.zeros(8)
    cases.append((z, z, np.zeros(8, dtype=np.uint64), np.zeros(8, dtype=np.uint64)))                        # nothing: NaN, NaN
    cases.append((z + 1.0, z, np.full(8, 3, dtype=np.uint64), np.full(8, 1, dtype=np.uint64)))              # a zero mean: NaN, not inf
    cases.append((np.array([1.0, np.nan, 2.0, 0.5]), np.array([1.0, 2.0, 0.0, 4.0]), np.array([2, 2, 2, 0], dtype=np.uint64), np.array([0, 0, 0, 2], dtype=np.uint64)))
    for EV, EM, PP, PU in cases:
        noise, coverage, rel = ref.derive(EV, EM, PP, PU)
        h_noise, h_coverage, h_rel = rmod.spectral_noise_derive(EV, EM, PP, PU)
        assert bits_equal(np.array([noise, coverage]), np.array([h_noise, h_coverage])) and bits_equal(rel, h_rel)
    assert math.isnan(h_noise) and h_coverage == 0.75 and np.isnan(h_rel[1:]).all() and h_rel[0] == math.sqrt(0.5) / 0.5
    assert math.isnan(rmod.spectral_noise_derive(*cases[2])[0])


def test_the_figure_is_sigma_over_root_n_over_mu():
    """iid Gaussian fluxes, mean mu, standard deviation sigma, exactly n samples in every sub-bin (sample k goes to sub-bin k % M).  Then e = s^2 / n with s^2 the
    sample variance of n values, and noise = sqrt(mean(s^2) / n) / mean(mu_hat).  Over K = H * W * B sub-bins mean(s^2) / sigma^2 has standard deviation
    sqrt(2 / (K (n - 1))), the square root halves it, and mean(mu_hat) / mu has standard deviation (sigma / mu) / sqrt(K n): the figure must equal
    sigma / sqrt(n) / mu within 4 times the sum of the two -- a bound of about 1.4 % here, which a ddof mistake (sqrt((n - 1) / n): 3 %), a factor of n or a
    variance in place of a standard error cannot meet."""
    H, W, bins, n, mu, sigma = 24, 24, 8, 16, 2.0, 0.5
    M, K = bins // 4, 24 * 24 * bins
    rng = np.random.default_rng(20250101)
    flux = rng.normal(mu, sigma, size=(H, W, n * M, 4)).astype(np.float32)
    centres = LMIN + (np.arange(M, dtype=np.float32) + np.float32(0.5)) * (LSTEP / np.float32(M))
    lam = np.broadcast_to(centres[np.arange(n * M) % M], (H, W, n * M)).astype(np.float32)
    S, Q, N = stats_ref.restate_sums(flux, lam, LMIN, LSTEP, bins)
    assert (N == n).all()
    noise, coverage = ref.figure(S, Q, N)
    want = sigma / math.sqrt(n) / mu
    bound = 4.0 * (math.sqrt(1.0 / (2.0 * K * (n - 1))) + (sigma / mu) / math.sqrt(K * n))
    print("figure", noise, "expected", want, "relative difference", noise / want - 1.0, "bound", bound)
    assert coverage == 1.0 and abs(noise / want - 1.0) <= bound, (noise, want, bound)


def test_the_csv_writer(tmp_path):
    EV = np.array([0.5, 1.0 / 3.0, 0.0, 2.0]); EM = np.array([1.5, -0.1, 0.0, 7.0])
    PP = np.array([3, 4, 2, 0], dtype=np.uint64); PU = np.array([0, 1, 2, 4], dtype=np.uint64)
    path = str(tmp_path / "n.csv")
    lmin, width = np.float32(380.0), np.float32(100.0 / 3.0)
    rmod.save_spectral_noise_csv(path, lmin, width, EV, EM, PP, PU)
    lines = open(path).read().split("\n")
    assert lines[0] == "bin,wavelength,rel,EV,EM,estimable,unestimated" and lines[-1] == "" and len(lines) == 2 + 4
    _, _, rel = ref.derive(EV, EM, PP, PU)
    for b in range(4):
        f = lines[1 + b].split(",")
        assert len(f) == 7 and (int(f[0]), int(f[5]), int(f[6])) == (b, int(PP[b]), int(PU[b]))
        assert np.float32(f[1]) == lmin + (np.float32(b) + np.float32(0.5)) * width                       # %.9g reads back to the same binary32
        for text, want in ((f[2], rel[b]), (f[3], EV[b]), (f[4], EM[b])):
            assert (text == "nan") if np.isnan(want) else (float(text) == want), (text, want)             # %.17g reads back to the same binary64
    assert lines[3].split(",")[2] == "nan" and lines[4].split(",")[2] == "nan"                            # a zero mean; nothing estimable
    with pytest.raises(rmod.SsxError):
        rmod.save_spectral_noise_csv(str(tmp_path / "no" / "dir.csv"), lmin, width, EV, EM, PP, PU)


@pytest.fixture(scope="module")
def cli():
    sbuild.build_host()
    assert os.path.exists(CLI)
    return CLI


def test_cli_refusals(cli, tmp_path):
    base = [cli, "-s=cornell-srgb", "-w=20", "-h=12", "-spp=4", "-o=" + str(tmp_path / "o.png"), "--texture=data/scenes/test-img.png"]
    target, full = "--spectral-noise-target=0.1", ["--spectral-noise-target=0.1", "--spectral-bins=8", "--max-samples=16"]

    def refused(args, *words):
        p = subprocess.run(base + args, cwd=ROOT, capture_output=True, text=True)
        assert p.returncode == 255 and "Simple Spectral" in p.stdout, (args, p.stderr)
        for w in words:
            assert w in p.stderr, (args, p.stderr)

    refused([target, "--max-samples=16"], "`--spectral-noise-target` needs `--spectral-bins=<n>`")
    refused([target, "--spectral-bins=8"], "`--spectral-noise-target` needs `--max-samples=<n>`")
    refused(full + ["--noise-target=0.1"], "`--spectral-noise-target` cannot be combined with `--noise-target`", "one stopping rule per run")
    refused(full + ["--resume=" + str(tmp_path / "c.ckpt")], "`--spectral-noise-target` cannot be combined with `--resume`", "does not carry the second moments")
    refused(full + ["--tile-major"], "`--spectral-noise-target` cannot be combined with `--tile-major`, `--rgb` or `--libm=glibc-2.35`")
    refused(full + ["--rgb"], "`--spectral-noise-target` cannot be combined with")
    refused(full + ["--libm=glibc-2.35"], "`--spectral-noise-target` cannot be combined with")
    for bad in ("x", "-1", "nan", "0.1x"):
        refused(["--spectral-noise-target=" + bad, "--spectral-bins=8", "--max-samples=16"], "Invalid value for --spectral-noise-target")
    for bad in ("x", "-0.1", "1.5", "nan"):
        refused(full + ["--spectral-noise-coverage=" + bad], "Invalid value for --spectral-noise-coverage")
    # the three companions need the rule
    refused(["--spectral-bins=8", "--spectral-noise-coverage=0.9"], "`--spectral-noise-coverage` needs `--spectral-noise-target=<x>`")
    refused(["--spectral-bins=8", "--spectral-noise-region=0,0,4,4"], "`--spectral-noise-region` needs `--spectral-noise-target=<x>`")
    refused(["--spectral-bins=8", "--spectral-noise-output=" + str(tmp_path / "n.csv")], "`--spectral-noise-output` needs `--spectral-noise-target=<x>`")
    # regions: --probe's words
    refused(full + ["--spectral-noise-region=4,0,4,4"], "`--spectral-noise-region=4,0,4,4` is empty or leaves the image: a rectangle is half-open")
    refused(full + ["--spectral-noise-region=0,5,4,3"], "is empty or leaves the image")
    refused(full + ["--spectral-noise-region=0,0,21,4"], "is empty or leaves the image")
    refused(full + ["--spectral-noise-region=0,0,4,4", "--spectral-noise-region=0,0,4,13"], "`--spectral-noise-region=0,0,4,13` is empty or leaves the image")
    refused(full + ["--spectral-noise-region=0,0,4"], "Invalid value for --spectral-noise-region (<x0>,<y0>,<x1>,<y1>)")
    refused(full + ["--spectral-noise-region=0,0,4,x"], "Invalid value for --spectral-noise-region")
    refused(full + ["--spectral-noise-region=-1,0,4,4"], "Invalid value for --spectral-noise-region")
    p = subprocess.run([cli], cwd=ROOT, capture_output=True, text=True)                 # the usage names the rule
    assert "--spectral-noise-target=<x>" in p.stdout and "--spectral-noise-region=<x0>,<y0>,<x1>,<y1>" in p.stdout
