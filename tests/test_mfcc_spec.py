"""mfcc.py without a device: Kaldi's DCT and lifter, what `KaldiMfcc` refuses, the specification `mfcc_host` against direct
formulas (the orthonormal DCT undone gives fbank's log-mel back; the energies against ln(sum of squares) computed here), the
float32 twin inside the bound dC, and the cap that keeps the GPU test's `|got - out| <= dC` from being vacuous: on the grid
tests/test_mfcc.py uses dC <= 1 for every element while the median of |out| is above 3."""
import os
import re

import numpy as np
import pytest

from test_fbank_spec import PATHS, paths_length

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (win, hop, filters, cepstra, L, snip_edges): tests/test_mfcc.py's grid
GRID = [(400, 160, 23, 13, 5000, True), (400, 160, 80, 80, 5000, False), (25, 10, 8, 5, 333, True), (16, 1, 4, 4, 40, True),
        (2048, 512, 40, 20, 9000, True)]
LN_FLOOR = np.log(2.0 ** -23)


def noise(rng, *shape):
    return rng.uniform(-1.0, 1.0, shape).astype(np.float32)


def test_dct_and_lifter():
    from alac.net_amd.mfcc import kaldi_dct, kaldi_lifter

    for n_ceps, n_mels in ((13, 23), (80, 80), (1, 1), (5, 8)):
        dct = kaldi_dct(n_ceps, n_mels)
        assert dct.dtype == np.float32 and dct.shape == (n_ceps, n_mels)
        m, c = np.arange(n_mels)[None, :], np.arange(n_ceps)[:, None]
        want = np.sqrt(2.0 / n_mels) * np.cos(np.pi / n_mels * (m + 0.5) * c)
        want[0] = np.sqrt(1.0 / n_mels)
        assert np.array_equal(dct, want.astype(np.float32))
        assert np.abs(dct.astype(np.float64) @ dct.astype(np.float64).T - np.eye(n_ceps)).max() <= 1e-6
        assert (dct[0] == dct[0, 0]).all()
    lifter = kaldi_lifter(13, 22)
    assert lifter.dtype == np.float32 and lifter[0] == 1.0
    assert np.array_equal(lifter, (1.0 + 11.0 * np.sin(np.pi * np.arange(13) / 22.0)).astype(np.float32))
    assert np.array_equal(kaldi_lifter(13, 0), np.ones(13, dtype=np.float32))
    for bad in (lambda: kaldi_dct(24, 23), lambda: kaldi_dct(0, 23), lambda: kaldi_lifter(13, -1.0), lambda: kaldi_lifter(13, float("nan"))):
        with pytest.raises(ValueError):
            bad()


def test_kaldimfcc_fields_and_refusals():
    import alac.net_amd as pkg
    from alac.net_amd.features import _Transform

    spec = pkg.KaldiMfcc(16000)
    assert isinstance(spec, _Transform) and not isinstance(spec, pkg.KaldiFbank)
    assert (spec.win_length, spec.hop_length, spec.n_filters, spec.n_ceps, spec.n_mels, spec.n_fft) == (400, 160, 23, 13, 13, 512)
    assert spec.cepstral_lifter == 22.0 and spec.use_energy is False and spec.raw_energy is True and spec.energy_floor == 0.0
    assert spec.fb.shape == (23, 257) and spec.dct.shape == (13, 23) and spec.lifter.shape == (13,)
    assert "use_energy=False is the default" in pkg.KaldiMfcc.__doc__
    for name in ("window", "basis", "fb", "dct", "lifter"):
        with pytest.raises(ValueError):
            getattr(spec, name)[0] = 0
    with pytest.raises(AttributeError):
        spec.n_ceps = 5
    fb = pkg.KaldiFbank(16000, n_mels=23)
    for name in ("window", "basis", "fb"):
        assert np.array_equal(getattr(spec, name), getattr(fb, name))
    assert spec.flags == 7 and pkg.KaldiMfcc(16000, use_energy=True).flags == 7 + 16 + 32
    assert pkg.KaldiMfcc(16000, use_energy=True, raw_energy=False, snip_edges=False).flags == 6 + 16
    assert pkg.KaldiMfcc(16000, raw_energy=True).flags == 7                                  # (32 goes with 16 only)
    assert spec.frames(32000) == 198 and spec.min_frames == 400 and fb.frames(32000) == 198
    assert spec.lengths(np.array([32000, 399, -1])).tolist() == [198, 0, -1]
    for kw in (dict(n_ceps=24), dict(n_ceps=0), dict(n_mels=5, n_ceps=6), dict(raw_energy=1), dict(raw_energy="yes"), dict(use_energy=0),
               dict(energy_floor=-1.0), dict(energy_floor=float("inf")), dict(cepstral_lifter=-2.0), dict(win_length=15), dict(scale=0.0),
               dict(log=True)):
        with pytest.raises((ValueError, TypeError)):
            pkg.KaldiMfcc(16000, **kw)
    with pytest.raises(ValueError):
        pkg.mfcc_host(np.zeros(1000, dtype=np.float32), fb)
    with pytest.raises(ValueError):
        pkg.mfcc_host(np.zeros(1000), spec)


def test_abi_is_mirrored():
    import alac.net_amd as pkg

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "alacgpu.h")).read(), flags=re.S)
    cs = open(os.path.join(ROOT, "alac.net_amd", "host", "csharp", "AlacGpuNative.cs")).read()
    for name, n_args, method in (("alacgpu_mfcc_device", 23, "mfcc_device"), ("alacgpu_deltas_device", 14, "deltas_device")):
        m = re.search(name + r"\s*\(([^)]*)\)", header)
        assert m and len(m.group(1).split(",")) == len(pkg.SYMBOLS[name][1]) == n_args
        m = re.search(name + r"\s*\(([^)]*)\)", cs)
        assert m and len(m.group(1).split(",")) == n_args, f"AlacGpuNative.cs does not declare {name} as the header does"
        assert hasattr(pkg.AlacGpuContext, method)


@pytest.mark.parametrize("snip", [True, False])
def test_square_dct_gives_the_log_mel_back(snip):
    import alac.net_amd as pkg

    x = noise(np.random.default_rng(1), 2, 3000)
    for use_power in (True, False):
        spec = pkg.KaldiMfcc(16000, n_mels=23, n_ceps=23, cepstral_lifter=0.0, snip_edges=snip, use_power=use_power)
        fb = pkg.KaldiFbank(16000, n_mels=23, snip_edges=snip, use_power=use_power)
        out = pkg.mfcc_host(x, spec)                                  # [2, 23, T]
        assert out.shape == (2, 23, spec.frames(3000))
        # the table is orthonormal as far as float32 goes (1e-7: its transpose gives the log-mel back to 1e-5 of values of
        # 20 or so), so the projection is undone by solving with the table itself: that holds 1e-9
        dct = spec.dct.astype(np.float64)
        want = pkg.fbank_host(x, fb)
        assert np.abs(np.einsum("cm,rct->rmt", dct, out) - want).max() <= 1e-4
        back = np.stack([np.linalg.solve(dct, o) for o in out])
        assert np.abs(back - want).max() <= 1e-9
    # n_ceps < n_mels is the first rows of the same projection, the lifter one product per line
    full = pkg.mfcc_host(x, pkg.KaldiMfcc(16000, n_mels=23, n_ceps=23, cepstral_lifter=0.0, snip_edges=snip))
    part = pkg.KaldiMfcc(16000, snip_edges=snip)
    assert np.abs(pkg.mfcc_host(x, part) - part.lifter.astype(np.float64)[None, :, None] * full[:, :13]).max() <= 1e-9


def test_the_energies():
    import alac.net_amd as pkg
    from alac.net_amd.fbank import fbank_frame_index

    x = noise(np.random.default_rng(2), 3000)
    kw = dict(remove_dc_offset=False, scale=1.0)
    spec = pkg.KaldiMfcc(16000, use_energy=True, raw_energy=True, **kw)
    idx = fbank_frame_index(3000, spec)
    fr = x.astype(np.float64)[idx]                                    # [T, 400]
    want = np.log(np.maximum((fr ** 2).sum(axis=1), 2.0 ** -23))
    out = pkg.mfcc_host(x, spec)
    plain = pkg.mfcc_host(x, pkg.KaldiMfcc(16000, **kw))
    assert np.abs(out[0] - want).max() <= 1e-12
    assert np.array_equal(out[1:], plain[1:]) and not np.array_equal(out[0], plain[0])     # C0 is replaced, nothing else
    # the windowed frame: ln(sum (window * preemphasised)^2)
    spec_w = pkg.KaldiMfcc(16000, use_energy=True, raw_energy=False, **kw)
    pre = fr - np.float64(np.float32(0.97)) * np.concatenate([fr[:, :1], fr[:, :-1]], axis=1)
    want_w = np.log(np.maximum(((spec_w.window.astype(np.float64) * pre) ** 2).sum(axis=1), 2.0 ** -23))
    assert np.abs(pkg.mfcc_host(x, spec_w)[0] - want_w).max() <= 1e-12
    assert np.abs(want_w - want).max() > 0.1
    # with the mean removed and Kaldi's scale the raw energy is that of d
    spec_d = pkg.KaldiMfcc(16000, use_energy=True)
    d = 32768.0 * fr
    d = d - d.mean(axis=1, keepdims=True)
    assert np.abs(pkg.mfcc_host(x, spec_d)[0] - np.log(np.maximum((d ** 2).sum(axis=1), 2.0 ** -23))).max() <= 1e-9
    # the floor: silent frames are ln(2^-23) without one, ln(energy_floor) with one; the comparison is in the log domain
    z = np.zeros(1000, dtype=np.float32)
    assert np.array_equal(pkg.mfcc_host(z, spec)[0], np.full(4, LN_FLOOR))
    floored = pkg.KaldiMfcc(16000, use_energy=True, energy_floor=0.5, **kw)
    assert np.array_equal(pkg.mfcc_host(z, floored)[0], np.full(4, float(np.float32(np.log(0.5)))))
    assert abs(floored.log_energy_floor - np.log(0.5)) <= 2.0 ** -24
    loud = pkg.mfcc_host(x, floored)[0]
    assert np.abs(loud - np.maximum(want, floored.log_energy_floor)).max() <= 1e-12 and (loud > floored.log_energy_floor).all()
    assert pkg.mfcc_host_f32(z, floored)[0].tolist() == [float(np.float32(np.log(0.5)))] * 4
    assert np.abs(pkg.mfcc_host_f32(z, spec)[0] - LN_FLOOR).max() <= 4 * 2.0 ** -24 * 17


def test_silence():
    import alac.net_amd as pkg

    spec = pkg.KaldiMfcc(16000)
    out, dC = pkg.mfcc_host(np.zeros((1, 1000), dtype=np.float32), spec, bound=True)
    want = spec.lifter.astype(np.float64) * LN_FLOOR * spec.dct.astype(np.float64).sum(axis=1)
    assert np.abs(out[0] - want[:, None]).max() <= 1e-12
    assert np.abs(pkg.mfcc_host_f32(np.zeros((1, 1000), dtype=np.float32), spec).astype(np.float64) - out).max() <= dC.max()


@pytest.fixture(scope="module")
def on_the_grid():
    """(out, dC, the twin's result) for every case of the grid and, with both values of snip_edges, of the code-path grid that
    tests/test_kaldi_paths.py runs on the device (tests/test_fbank_spec.py: PATHS), computed once"""
    import alac.net_amd as pkg

    res = {}
    for win, hop, n_mels, n_ceps, L, snip in GRID:
        spec = pkg.KaldiMfcc(16000, win, hop, n_mels, n_ceps, snip_edges=snip)
        x = noise(np.random.default_rng(win), 1, L)
        out, dC = pkg.mfcc_host(x, spec, bound=True)
        res[win, n_mels] = (out, dC, pkg.mfcc_host_f32(x, spec))
    for win, hop, n_mels, n_ceps, frames in PATHS:
        x = noise(np.random.default_rng(win + hop), 1, paths_length(win, hop, frames))
        for snip in (True, False):
            spec = pkg.KaldiMfcc(16000, win, hop, n_mels, n_ceps, snip_edges=snip)
            out, dC = pkg.mfcc_host(x, spec, bound=True)
            res["paths", win, hop, n_mels, snip] = (out, dC, pkg.mfcc_host_f32(x, spec))
    return res


def test_the_twin_is_inside_the_bound(on_the_grid):
    for key, (out, dC, twin) in on_the_grid.items():
        assert twin.dtype == np.float32 and twin.shape == out.shape
        err = np.abs(twin.astype(np.float64) - out)
        print(f"{key}: max err {err.max():.3e}, max err / dC {np.max(err / dC):.4f}")
        assert (err <= dC).all(), key
        # a float32 evaluation of values of a few units -- but for 256 filters at 2048 taps, the one shape whose dC is not
        # below 1 (test_the_bound_is_not_vacuous says why): the logs of its lowest filters are ill-conditioned for the twin too
        assert err.max() <= 2e-4 or key[:4] == ("paths", 2048, 560, 256), key


def test_the_bound_is_not_vacuous(on_the_grid):
    """(2048, 560, 256, 23) of PATHS stays out: 256 filters over 1025 bins are a few bins each, pre-emphasis leaves the lowest
    of them little power, their logs' intervals are wide and dC reaches 3.4 -- the condition below does not hold there, so
    tests/test_kaldi_paths.py does not use dC for that shape (it holds the cepstra to the DCT of the fbank kernel's bits)"""
    assert ("paths", 2048, 560, 256, True) in on_the_grid
    for key, (out, dC, _) in on_the_grid.items():
        if key[:4] == ("paths", 2048, 560, 256):
            continue
        print(f"{key}: max dC {dC.max():.4f}, median |out| {np.median(np.abs(out)):.2f}")
        assert (dC > 0).all() and dC.max() <= 1.0, key
        assert np.median(np.abs(out)) > 3.0, key


def test_the_energy_bound_and_twin():
    import alac.net_amd as pkg

    x = noise(np.random.default_rng(3), 2, 3000) + np.float32(0.1)
    for kw in (dict(raw_energy=True), dict(raw_energy=False), dict(raw_energy=True, remove_dc_offset=False), dict(energy_floor=1e9)):
        spec = pkg.KaldiMfcc(16000, use_energy=True, **kw)
        out, dC = pkg.mfcc_host(x, spec, bound=True)
        err = np.abs(pkg.mfcc_host_f32(x, spec).astype(np.float64) - out)
        print(f"{kw}: E {out[0, 0, 0]:.4f}, dE {dC[:, 0].max():.3e}, twin {err[:, 0].max():.3e}")
        assert (err <= dC).all() and dC[:, 0].max() <= 1e-3, kw
