"""The float32 twin of the phase vocoder held to the float64 specification one stage at a time, without a device
(alac.net_amd/pitch.py): each of `analyse_host_f32`, `scan_host_f32` and `synthesise_host_f32` against the float64 stage applied
to the twin's own float32 input of that stage, cast up, within that stage's bound for exact inputs.  The end-to-end bound of
tests/test_stretch_spec.py has to absorb the vocoder's own condition (a bin that is small in one frame loses its phase) and so
lets through errors of a good share of the peak; a single stage from the same input is off by rounding only, and its bound is
orders of magnitude tighter.  tests/test_stretch.py and tests/test_stretch_paths.py carry the twin to the kernels bit for bit.

Every check also asks that some of the bound is used: a yardstick that is never approached measures nothing.  The mutants are
the twin's scan and synthesis restated here with one switch each (the unswitched restatements equal the twin's bits); every
mutant has to fail a staged check.  One of them -- the imaginary parts of the bins 0 and N / 2 kept -- cannot show in y at
all: the scan makes those parts exactly zero, and whatever stands there reaches only the imaginary part of the inverse
transform, bit for bit (the two bins lie where no stage of the inverse multiplies by a twiddle).  What the synthesis promises
about them is a statement about the spectrum of N points it hands to the inverse transform, so that piece of the stage
(`hermitian_host_f32`, a copy without arithmetic) is held to its float64 statement exactly, on the twin's Y with imaginary
parts planted in the two bins.

With ALAC_STRETCH_PROFILES=1 in the environment the measured shares go to profiles/stretch_stages.json and the mutant table to
profiles/stretch_mutants.txt."""
import json
import os
from fractions import Fraction as F

import numpy as np
import pytest

from test_stretch_spec import signal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACTORS = (F(1, 2), F(2), F(9, 10), F(11, 10), F(200, 189))
LONG = (512, F(2), 1, 32000)                                # about 500 chained frames: the linear drift term at its largest
FLOOR = 2.0 ** -60                                          # every bin above it: no square underflows, the derivation's premise
FILL = "the spectrum of N points"                           # a copy: held exactly, it has no share of a bound
STAGES = ("analyse", "scan", "synthesise")


@pytest.fixture(scope="module")
def pitch():
    import alac.net_amd.pitch as m

    return m


def cases(pitch):
    """(n_fft, factor, channels, frames): the shortest live row, about three transforms, and the long one"""
    out = [(n_fft, f, C, T) for n_fft in pitch.N_FFTS for f in FACTORS for C in (1, 2) for T in (n_fft // 2 + 1, 3 * n_fft + 17)]
    return out + [LONG]


def up(z):
    return z[0].astype(np.float64) + 1j * z[1].astype(np.float64)


def share(err, bound):
    """The largest err / bound; where the bound is 0 the error has to be"""
    assert not err[bound == 0].any()
    return float((err[bound > 0] / bound[bound > 0]).max())


def spectrum(pitch, Y):
    """The float64 statement of `hermitian_host_f32`: what irfft takes Y complex [C, T', K] for, at the kernel's positions"""
    C, Tp, K = Y.shape
    N = 2 * (K - 1)
    pos = pitch.positions(N)
    S = np.zeros((C * Tp, N), dtype=np.complex128)
    Y = Y.reshape(C * Tp, K)
    k = np.arange(1, K - 1)
    S[:, pos[k]], S[:, pos[N - k]] = Y[:, k], np.conj(Y[:, k])
    S[:, pos[0]], S[:, pos[N // 2]] = Y[:, 0].real, Y[:, K - 1].real
    return S


def staged(pitch, x, p, q, n_fft, scan=None, synthesise=None, fill=None):
    """The staged checks of one row: {stage: the worst share of its bound}, and what the tightness record needs.  scan,
    synthesise, fill: stand-ins for the twin's stage functions (the mutants); the stage's input is always the twin's own."""
    scan, synthesise, fill = scan or pitch.scan_host_f32, synthesise or pitch.synthesise_host_f32, fill or pitch.hermitian_host_f32
    v = x.shape[1]
    T = pitch.stft_frames(v, n_fft)
    out, sizes = {}, {}
    X32 = pitch.analyse_host_f32(x, n_fft)
    X64, e = pitch.analyse_host(x, n_fft), pitch.analyse_bound(x, n_fft)
    err = np.sqrt((np.abs(up(X32) - X64) ** 2).sum(axis=-1))
    out["analyse"] = share(err, e)
    sizes["analyse"] = float(e.max() / np.sqrt((np.abs(X64) ** 2).sum(axis=-1)).max())
    Xin = up(X32)
    assert np.abs(Xin[:, :T]).min() > FLOOR                  # the premise, from the float64 X
    Y32 = pitch.scan_host_f32(X32, p, q)
    Y64, dY = pitch.scan_host(Xin, p, q), pitch.scan_bound(Xin, p, q)
    out["scan"] = share(np.abs(up(scan(X32, p, q)) - Y64), dY)
    sizes["scan"] = float(dY.max() / np.abs(Y64).max())
    Yin = up(Y32)
    y64, dy = pitch.synthesise_host(Yin, v, p, q), pitch.synthesise_bound(Yin, v, p, q)
    out["synthesise"] = share(np.abs(synthesise(Y32, v, p, q).astype(np.float64) - y64), dy)
    sizes["synthesise"], sizes["largest staged dy"] = float(dy.max() / np.abs(y64).max()), float(dy.max())
    planted = (Y32[0], Y32[1].copy())                       # imaginary parts in the bins 0 and N / 2, which the scan leaves at zero
    planted[1][..., 0], planted[1][..., -1] = Y32[0][..., 0], -Y32[0][..., -1]
    out[FILL] = 0.0 if np.array_equal(up(fill(planted)), spectrum(pitch, up(planted))) else float("inf")
    return out, sizes


@pytest.fixture(scope="module")
def records(pitch):
    """Every case once: [(case, shares, sizes of the staged bounds, the end-to-end bound's, the synthesis bound's largest)]"""
    out = []
    for n_fft, f, C, T in cases(pitch):
        x = signal(7 * n_fft + T + C, C, T)
        p, q = f.numerator, f.denominator
        shares, sizes = staged(pitch, x, p, q, n_fft)
        y, dy = pitch.vocoder_host(x, p, q, n_fft, bound=True)
        sizes["end to end"], sizes["largest end-to-end dy"] = float(dy.max() / np.abs(y).max()), float(dy.max())
        out.append(((n_fft, f, C, T), shares, sizes))
    return out


@pytest.mark.parametrize("stage", STAGES)
def test_the_twins_stage_is_within_the_stage_bound_and_uses_some_of_it(records, stage):
    for case, shares, _ in records:
        assert 0 < shares[stage] <= 1, (case, shares[stage])
        assert shares[FILL] == 0, case                      # (exact or not)
    for n_fft in sorted({c[0][0] for c in records}):
        print(f"{stage}, n_fft {n_fft}: at most {max(s[stage] for c, s, _ in records if c[0] == n_fft):.3g} of the stage's bound")


def test_the_staged_bound_is_below_the_end_to_end_bound(records):
    """The staged synthesis bound and the end-to-end dy, both as fractions of the row's peak; the fractions are the record."""
    rows = []
    for (n_fft, f, C, T), shares, sizes in records:
        assert sizes["largest staged dy"] < sizes["largest end-to-end dy"], (n_fft, f, C, T)
        rows.append({"n_fft": n_fft, "factor": str(f), "channels": C, "frames": T,
                     "share_of_the_stage_bound": {k: shares[k] for k in STAGES},
                     "bound_over_peak": {k: sizes[k] for k in ("analyse", "scan", "synthesise", "end to end")}})
    worst = {str(n_fft): {k: max(s[k] for c, s, _ in records if c[0] == n_fft) for k in STAGES} for n_fft in (512, 1024, 2048)}
    ratio = min(r["bound_over_peak"]["end to end"] / r["bound_over_peak"]["synthesise"] for r in rows)
    print(json.dumps(worst, indent=1))
    print(f"the end-to-end bound is at least {ratio:.3g} times the staged synthesis bound")
    if os.environ.get("ALAC_STRETCH_PROFILES") == "1":
        doc = {"what": "tests/test_stretch_stages.py: the share of each stage's bound that the float32 twin uses against the float64 "
                       "stage on the same input, and each bound's largest value over the row's largest value (analyse: e_t over "
                       "the largest frame norm; scan: dY over the largest |Y|; synthesise and end to end: dy over the peak)",
               "worst_share_by_n_fft": worst, "least_end_to_end_over_staged_synthesis": ratio, "cases": rows}
        with open(os.path.join(ROOT, "profiles", "stretch_stages.json"), "w") as fh:
            json.dump(doc, fh, indent=1)
            fh.write("\n")


# ---- the mutants ----------------------------------------------------------------------------------------------------------------
SCAN_MUTANTS = ("the weights alpha and 1 - alpha swapped", "P_0 = (1, 0) instead of ph(X_0)",
                "ph(a) conj(ph(b)) instead of ph(b) conj(ph(a))", "the frame pair read at i - 1, i instead of i, i + 1")
SYNTH_MUTANTS = ("the Hermitian half filled without the conjugate", "the imaginary parts of bins 0 and N/2 kept",
                 "the envelope without the last covering frame", "the window applied once, at analysis only")


def scan32(pitch, X, p, q, mutant=None):
    """`scan_host_f32` restated, with the scan's mutants"""
    f32 = np.float32
    Xr, Xi = X
    C, T2, K = Xr.shape
    i, num = pitch.steps(T2 - 2, p, q)
    alpha = num.astype(f32) / f32(p)
    Yr, Yi = np.zeros((C, len(i), K), dtype=f32), np.zeros((C, len(i), K), dtype=f32)
    P = pitch._ph32((Xr[:, 0], Xi[:, 0]))
    if mutant == SCAN_MUTANTS[1]:
        P = (np.ones((C, K), dtype=f32), np.zeros((C, K), dtype=f32))
    zero = (np.zeros((C, K), dtype=f32), np.zeros((C, K), dtype=f32))
    frame = lambda t: zero if t < 0 else (Xr[:, t], Xi[:, t])
    for j in range(len(i)):
        a, b = (frame(i[j] - 1), frame(i[j])) if mutant == SCAN_MUTANTS[3] else (frame(i[j]), frame(i[j] + 1))
        wb, wa = (f32(1) - alpha[j], alpha[j]) if mutant == SCAN_MUTANTS[0] else (alpha[j], f32(1) - alpha[j])
        mag = wb * pitch._abs32(b) + wa * pitch._abs32(a)
        Yr[:, j], Yi[:, j] = mag * P[0], mag * P[1]
        pa, pb = pitch._ph32(a), pitch._ph32(b)
        d = pitch._cmul(pa, (pb[0], -pb[1])) if mutant == SCAN_MUTANTS[2] else pitch._cmul(pb, (pa[0], -pa[1]))
        P = pitch._ph32(pitch._cmul(P, d))
    return Yr, Yi


def fill32(pitch, Y, mutant=None):
    """`hermitian_host_f32` restated, with its mutants"""
    f32 = np.float32
    Yr, Yi = Y
    C, Tp, K = Yr.shape
    N = 2 * (K - 1)
    pos = pitch.positions(N)
    zr, zi = np.zeros((C * Tp, N), dtype=f32), np.zeros((C * Tp, N), dtype=f32)
    zr[:, pos[:K]] = Yr.reshape(C * Tp, K)
    if mutant == SYNTH_MUTANTS[1]:
        zi[:, pos[:K]] = Yi.reshape(C * Tp, K)
    else:
        zi[:, pos[1:K - 1]] = Yi.reshape(C * Tp, K)[:, 1:K - 1]
    mirror = pos[N - np.arange(1, K - 1)]
    zr[:, mirror] = Yr.reshape(C * Tp, K)[:, 1:K - 1]
    zi[:, mirror] = (1 if mutant == SYNTH_MUTANTS[0] else -1) * Yi.reshape(C * Tp, K)[:, 1:K - 1]
    return zr, zi


def synthesise32(pitch, Y, v, p, q, mutant=None):
    """`synthesise_host_f32` restated, with the synthesis' mutants"""
    f32 = np.float32
    C, Tp, K = Y[0].shape
    N = 2 * (K - 1)
    H = N // 4
    w, tw = pitch.window(N, f32), pitch.twiddles(N)
    zr, zi = fill32(pitch, Y, mutant)
    pitch._inverse(zr, zi, tw)
    scaled = zr * f32(1.0 / N)
    fr = (scaled if mutant == SYNTH_MUTANTS[3] else w * scaled).reshape(C, Tp, N)
    total = (Tp - 1) * H + N
    acc, env = np.zeros((C, total), dtype=f32), np.zeros(total, dtype=f32)
    w2 = w * w
    for j in range(Tp):
        acc[:, j * H:j * H + N] += fr[:, j]
        if mutant == SYNTH_MUTANTS[2]:                     # a frame's first hop is where it is the last to cover a sample
            env[j * H + H:j * H + N] += w2[H:]
        else:
            env[j * H:j * H + N] += w2
    Ls = pitch.stretched_frames(v, p, q)
    n = min(Ls, (Tp - 1) * H + 1)
    y = np.zeros((C, Ls), dtype=f32)
    y[:, :n] = acc[:, N // 2:N // 2 + n] / env[N // 2:N // 2 + n]
    return y


def mutant_rows(pitch):
    return [(n_fft, f, 1, 3 * n_fft + 17) for n_fft in pitch.N_FFTS for f in (F(11, 10), F(1, 2))]


def test_the_restated_stages_are_the_twins(pitch):
    for n_fft, f, C, T in mutant_rows(pitch):
        x = signal(T, 2, T)
        p, q = f.numerator, f.denominator
        X = pitch.analyse_host_f32(x, n_fft)
        Y = pitch.scan_host_f32(X, p, q)
        mine = scan32(pitch, X, p, q)
        assert np.array_equal(mine[0].view(np.int32), Y[0].view(np.int32)) and np.array_equal(mine[1].view(np.int32), Y[1].view(np.int32))
        y = synthesise32(pitch, Y, T, p, q)
        assert np.array_equal(y.view(np.int32), pitch.synthesise_host_f32(Y, T, p, q).view(np.int32))
        for mine, twins in zip(fill32(pitch, Y), pitch.hermitian_host_f32(Y)):
            assert np.array_equal(mine.view(np.int32), twins.view(np.int32))
        assert np.array_equal(y.view(np.int32), pitch.vocoder_host_f32(x, p, q, n_fft).view(np.int32))


@pytest.fixture(scope="module")
def parents_cases(pitch):
    """The cases of test_stretch_spec's end-to-end test with the specification and its bound, computed once"""
    from test_stretch_spec import FACTORS as ORDER

    out = []
    for n_fft, T, C in ((512, 4000, 2), (1024, 3000, 1), (2048, 5000, 1)):
        x = np.stack([signal(10 * n_fft + b, C, T) for b in range(len(ORDER))])
        lengths = [T, T - 77, T // 2 + 100, T - 1, n_fft // 2 + 1]
        y, _, dy = pitch.time_stretch_host(x, list(ORDER), lengths, n_fft, bound=True)
        out.append((x, list(ORDER), lengths, n_fft, y, dy))
    return out


def end_to_end(pitch, parents_cases, scan, synthesise):
    """The parent's check on a twin with these stages: the largest err / dy over its cases (above 1: it catches the mutant)"""
    worst = 0.0
    for x, factors, lengths, n_fft, y, dy in parents_cases:
        row = lambda xr, p, q, N: synthesise(scan(pitch.analyse_host_f32(xr, N), p, q), xr.shape[1], p, q)
        y32, _ = pitch._rows(x, factors, lengths, n_fft, row, np.float32)
        err = np.abs(y32.astype(np.float64) - y)
        if (err[dy == 0] != 0).any() or not np.isfinite(err).all():
            return float("inf")
        worst = max(worst, float((err[dy > 0] / dy[dy > 0]).max()))
    return worst


def test_every_mutant_fails_a_staged_check(pitch, parents_cases):
    from functools import partial

    assert end_to_end(pitch, parents_cases, pitch.scan_host_f32, pitch.synthesise_host_f32) <= 1
    lines = ["tests/test_stretch_stages.py: each mutant of the twin's scan or synthesis against the staged checks (the worst",
             "error over the stage's bound, over three n_fft and the factors 11/10 and 1/2) and against the end-to-end check of",
             "tests/test_stretch_spec.py (err <= dy over its own cases).  Above 1 fails the check.", ""]
    for k, mutant in enumerate(SCAN_MUTANTS + SYNTH_MUTANTS):
        scan = partial(scan32, pitch, mutant=mutant) if k < 4 else pitch.scan_host_f32
        synth = partial(synthesise32, pitch, mutant=mutant) if k >= 4 else pitch.synthesise_host_f32
        fill = partial(fill32, pitch, mutant=mutant) if k >= 4 else pitch.hermitian_host_f32
        worst = {}
        for n_fft, f, C, T in mutant_rows(pitch):
            shares, _ = staged(pitch, signal(T, C, T), f.numerator, f.denominator, n_fft, scan, synth, fill)
            for stage, s in shares.items():
                worst[stage] = max(worst.get(stage, 0.0), s)
        failed = {stage: s for stage, s in worst.items() if not s <= 1}
        whole = end_to_end(pitch, parents_cases, scan, synth)
        lines.append(f"{mutant}")
        lines.append("    staged:     " + ("; ".join(f"{stage} differs (a copy: it is held exactly)" if stage == FILL else f"{stage} fails at {s:.3g} times its bound"
                                                   for stage, s in failed.items()) or "passes"))
        lines.append(f"    end to end: {'fails' if whole > 1 else 'passes'} at {whole:.3g} times its bound")
        print("\n".join(lines[-3:]))
        assert failed, mutant
    if os.environ.get("ALAC_STRETCH_PROFILES") == "1":
        with open(os.path.join(ROOT, "profiles", "stretch_mutants.txt"), "w") as fh:
            fh.write("\n".join(lines) + "\n")
