"""The encoder policy reference (encode_ref.py) on the CPU: its LPC against the synth encoder's own Levinson-Durbin, its
choices on hand-built signals, its float64 error bound, and its sample conversion on a table of edge values."""
import numpy as np
import pytest

import encode_ref as er
import test_encode as te


def synth_lpc(synth, stream_pcm, ss, stereo):
    """The synth's own quantised LPC (coef_mode 0, mix weight 0): channel A's and B's coefficients from its header."""
    n = len(stream_pcm) // (2 if stereo else 1)
    cfg = (4096, ss, 40, 10, 14, 2 if stereo else 1)
    d = er.desc(synth, n, cfg, ub=1 if ss == 24 else 0, coef_mode=0, mix_shift=2 if stereo else 0, mix_weight=0)
    pkt = synth.encode_packet(d, stream_pcm)
    got, _, _ = te.recipe(synth, pkt, cfg)
    return [list(got["coefs"][0, c, :8]) for c in range(2 if stereo else 1)]


@pytest.mark.parametrize("n", [10, 513, 4096])
@pytest.mark.parametrize("ss", [16, 24])
def test_lpc_equals_synth_levinson(synth, n, ss):
    """Where a L + b R is exact (mono; L and R at weight 0), the exact Levinson-Durbin quantises like the synth's float64 one."""
    seen = 0
    for seed in range(6):
        sig = synth.default_signal(100 + seed)
        sig["silence_prob"] = 0.3
        for C_ in (1, 2):
            pcm = synth.make_pcm(sig, seed * 7 + n, ss, C_, n)
            ref = er.reference_packet(synth, pcm.reshape(-1, C_), (4096, ss, 40, 10, 14, C_))
            assert ref.firm
            want = synth_lpc(synth, pcm, ss, C_ == 2)
            assert ref.coefs[0] == want[0], (seed, C_)
            if C_ == 2:
                assert ref.coefs[1] == want[1], seed
            seen += any(ref.coefs[0])
    assert seen >= 6   # the signals do have coefficients


def tone_dc_signals(ss, n=4096, k=4, seed=0):
    """Pure tones and DC with silence, stereo: the ill-conditioned correlation matrices."""
    rng = np.random.default_rng(seed + ss)
    lim = (1 << (ss - 1)) - 1
    i = np.arange(n)
    out = []
    for j in range(k):
        f = rng.uniform(0.001, 0.3)
        tone = np.stack([np.round(lim * 0.7 * np.sin(f * i + j)), np.round(lim * 0.4 * np.sin(f * i + 1))], 1)
        dc = np.stack([np.full(n, rng.integers(-lim, lim)), np.full(n, rng.integers(-lim, lim))], 1)
        a = int(rng.integers(0, n - n // 4))
        dc[a:a + n // 4] = 0
        out += [tone.astype(np.int32), dc.astype(np.int32)]
    return out


@pytest.mark.parametrize("ss", [16, 24])
def test_float64_error_is_small(synth, ss):
    """The plain float64 Levinson-Durbin's c * 512 against the exact value, over synth signals, tones and DC: measured at
    most about 1.3e-8 (tones), so delta = 64 * err64 is far inside GUARD."""
    worst = 0.0
    sigs = tone_dc_signals(ss) + [synth.make_pcm(synth.default_signal(3), p, ss, 2, 4096).reshape(-1, 2) for p in range(8)]
    for pcm in sigs:
        ref = er.reference_packet(synth, pcm, (4096, ss, 40, 10, 14, 2))
        worst = max(worst, ref.err64)
        assert ref.firm
    assert 0 < worst < 1e-6, worst
    assert er.DELTA_FACTOR * 1e-6 < er.GUARD


def test_auto_mode_matches_exact(synth):
    for p in range(6):
        pcm = synth.make_pcm(synth.default_signal(21), p, 16, 2, 2000).reshape(-1, 2)
        a = er.reference_packet(synth, pcm, (4096, 16, 40, 10, 14, 2))
        b = er.reference_packet(synth, pcm, (4096, 16, 40, 10, 14, 2), exact="auto")
        assert a.packet == b.packet and a.coefs == b.coefs and a.firm == b.firm


def stereo(l, r):
    return np.ascontiguousarray(np.stack([l, r], 1).astype(np.int32))


def music(n=4096, seed=1, amp=3000.0):
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    return np.round(amp * np.sin(0.013 * i) + amp / 3 * np.sin(0.21 * i + 1) + rng.normal(0, 40, n))


@pytest.mark.parametrize("ss", [16, 24])
def test_choice_l_equals_r(synth, ss):
    x = music() * (256 if ss == 24 else 1)
    ref = er.reference_packet(synth, stereo(x, x), (4096, ss, 40, 10, 14, 2))
    assert ref.coefs[er.NS - 1] == [0] * 8                     # B = L - R is silent
    assert ref.nbits[1] == ref.nbits[2] == ref.nbits[3] == ref.nbits[4] < ref.nbits[0]   # every A_w is R: a tie
    assert ref.weight == 1 and not ref.escape                  # the smaller weight wins


def test_choice_l_equals_minus_r(synth):
    x = music()
    ref = er.reference_packet(synth, stereo(x, -x), (4096, 16, 40, 10, 14, 2))
    assert ref.coefs[3] == [0] * 8                             # A_2 = R + ((L - R) * 2 >> 2) = 0
    assert ref.weight == 2
    assert_choice_rule(ref)


def assert_choice_rule(ref):
    """The smallest usable bit count wins, the first (smallest) weight among equals."""
    usable = [b for b in ref.nbits if b is not None]
    assert ref.nbits[ref.weight] == min(usable) and ref.nbits.index(min(usable)) == ref.weight


@pytest.mark.parametrize("silent", [0, 1])
def test_choice_one_silent_channel(synth, silent):
    x = music(seed=4)
    l, r = (0 * x, x) if silent == 0 else (x, 0 * x)
    ref = er.reference_packet(synth, stereo(l, r), (4096, 16, 40, 10, 14, 2))
    assert ref.coefs[silent] == [0] * 8 and not ref.escape
    assert_choice_rule(ref)
    if silent == 1:
        assert ref.weight == 0                                 # L and a silent R beat any mix with L in both streams


def test_choice_tie_goes_to_smaller_weight(synth):
    """Digital silence: every weight writes the same bits; weight 0 wins."""
    ref = er.reference_packet(synth, np.zeros((500, 2), np.int32), (4096, 16, 40, 10, 14, 2))
    assert len(set(ref.nbits)) == 1 and ref.weight == 0


@pytest.mark.parametrize("ss,C_", [(16, 2), (24, 1)])
def test_full_scale_noise_escapes(synth, ss, C_):
    lo, hi = er.sample_range(ss)
    pcm = np.random.default_rng(5).integers(lo, hi + 1, (4096, C_)).astype(np.int32)
    ref = er.reference_packet(synth, pcm, (4096, ss, 40, 10, 14, C_))
    assert ref.escape and ref.margin is not None and ref.margin <= 0
    d = er.desc(synth, 4096, (4096, ss, 40, 10, 14, C_), escape=1)
    assert ref.packet == synth.encode_packet(d, pcm.reshape(-1))


@pytest.mark.parametrize("kb,usable", [(31, True), (32, False), (33, True), (64, False)])
def test_zero_runs_under_kb(synth, kb, usable):
    """kb a multiple of 32: the zero-run count's mask is 0, so a candidate with a silent stretch is unusable."""
    x = music(seed=8)
    x[1000:1600] = 0
    for C_ in (1, 2):
        pcm = stereo(x, x // 2) if C_ == 2 else x.astype(np.int32).reshape(-1, 1)
        ref = er.reference_packet(synth, pcm, (4096, 16, 40, 10, kb, C_))
        if usable:
            assert not ref.escape and ref.nbits[ref.weight] is not None
        else:
            assert all(b is None for b in ref.nbits) and ref.escape and ref.margin is None


F32 = np.float32


def conversion_table(ss):
    """(input, expected canonical sample) for int32 and float32 input at sample size ss."""
    lo, hi = er.sample_range(ss)
    s = F32(1 << (ss - 1))
    ints = [(2 ** 31 - 1, hi), (-2 ** 31, lo), (hi + 1, hi), (lo - 1, lo), (hi, hi), (lo, lo), (0, 0), (-1, -1), (12345, 12345)]
    floats = [
        (F32(0.0), 0), (F32(-0.0), 0), (F32(1e-45), 0), (F32(-1e-45), 0), (F32(1.2e-38), 0),
        (F32(1.0), hi), (F32(-1.0), lo), (F32(2.0), hi), (F32(-3.5), lo), (F32(np.inf), hi), (F32(-np.inf), lo),
        (F32(np.nan), lo), (F32(-np.nan), lo),
        (F32(1) / s, 1), (F32(-3) / s, -3), (F32(hi) / s, hi),                          # grid points
        (F32(0.5) / s, 0), (F32(1.5) / s, 2), (F32(2.5) / s, 2), (F32(-0.5) / s, 0),    # half-LSB ties: to even
        (F32(-1.5) / s, -2), (F32(-2.5) / s, -2), (F32(1001.5) / s, 1002),
        (np.nextafter(F32(2.5) / s, F32(0)), 2), (np.nextafter(F32(2.5) / s, F32(1)), 3),
        (np.nextafter(F32(-2.5) / s, F32(0)), -2), (np.nextafter(F32(-2.5) / s, F32(-1)), -3),
        (np.nextafter(F32(1.0), F32(0)), hi), (np.nextafter(F32(-1.0), F32(0)), lo),
    ]
    if ss == 16:
        floats += [(F32(hi + 0.5) / s, hi), (F32(lo - 0.5) / s, lo)]   # clamped before the rounding
    return ints, floats


@pytest.mark.parametrize("ss", [16, 24])
def test_conversion_table(ss):
    ints, floats = conversion_table(ss)
    got = er.convert(np.array([v for v, _ in ints], np.int32), ss)
    assert got.tolist() == [e for _, e in ints]
    got = er.convert(np.array([v for v, _ in floats], np.float32), ss)
    assert got.tolist() == [e for _, e in floats]
