"""alacgpu_logmel_device on the GPU against its specification in numpy (features.logmel_host), element by element.  The
tolerance is the derived one of features.py: with u = 2^-24 and a_n = |window[n] x_t[n]|,
    delta_j = (n_fft + 2) u sum_n a_n |basis[n, j]|        one rounding of the window product, a chain of n_fft fmas
    dP_k    = 2 |Re| delta_re + delta_re^2 + 2 |Im| delta_im + delta_im^2 + 3 u P_k
    dM_m    = sum_k fb[m, k] dP_k + (n_bins + 1) u M_m
In the power domain |got - M| <= dM.  With a log, got must lie in [log(max(M - dM, floor)) - e, log(max(M + dM, floor)) + e],
e = 4 u (|log value| + 1) for logf; those tests use full-scale noise and first assert dM / M <= 0.1 on their own input, so the
interval is narrow.  Tonal, impulse, silent and tiny inputs (most of whose mel power is float32 leakage below the floor) are
compared in the power domain; silence with a log must give log(floor) in every element.

dM is a bound on every float32 evaluation and 20 to 1000 times wider than the error of a correct one, so on full-scale noise
there is a second, tight yardstick (check_power(..., twin=True)): features.logmel_host_f32, the kernel's arithmetic one float32
operation at a time on the CPU.  With r_ref = max |twin - M| / dM and r_gpu = max |got - M| / dM over the same input,
r_gpu <= 4 r_ref: both are float32 evaluations with the same number of roundings per element; another association inside a
two-tap MFMA step or flushed denormals change individual roundings, not their count, and the maxima of two such samples over
thousands of elements differ by far less than a factor of 2.  The yardstick is the reference's own error, never the kernel's.
tests/test_features_paths.py runs the same checks over a grid of shapes chosen by the kernel's branches."""
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
GUARD = 64
SHAPES = [(400, 160, 80, 5000), (25, 10, 8, 333), (16, 1, 4, 40), (512, 128, 64, 4000), (2048, 512, 128, 9000)]


def header_constant(name, file="alac_features.h"):
    src = open(os.path.join(ROOT, "alac.net_amd", "csrc", file)).read()
    m = re.search(r"constexpr\s+(?:uint32_t|size_t|int)\s+" + name + r"\s*=\s*(\d+)u?\s*(?:<<\s*(\d+))?\s*;", src)
    assert m, f"{file} does not define {name}"
    return int(m.group(1)) << int(m.group(2) or 0)


def kernel_tile(n_fft, hop):
    """alac_features_tile of alac_features.h"""
    tile, most = header_constant("ALAC_FEATURES_TILE"), header_constant("ALAC_FEATURES_MAX_SPAN")
    return tile if (tile - 1) * hop + n_fft <= most else 1 + (most - n_fft) // hop


def kernel_blocks(n_fft):
    """the blocks of ALAC_FEATURES_BLOCK bins a workgroup goes through"""
    return -(-(n_fft // 2 + 1) // header_constant("ALAC_FEATURES_BLOCK"))


def kernel_lds_bytes(n_fft, hop, n_mels):
    """alac_features_lds_layout(...).bytes() of alac_features.h: window, mel sums, the power of a round, the skewed span"""
    tile, block, per_round = (header_constant("ALAC_FEATURES_" + n) for n in ("TILE", "BLOCK", "ROUND_BLOCKS"))
    span = (kernel_tile(n_fft, hop) - 1) * hop + n_fft
    skewed = span + (0 if hop & 1 else (span - 1) // hop + 1)
    return 4 * (((n_fft + 3) & ~3) + n_mels * tile + min(kernel_blocks(n_fft), per_round) * block * tile + skewed)


def specs(n_fft, hop, n_mels, sample_rate=16000, **kw):
    """The transform with no log, ln and log10"""
    from alac.net_amd.features import LogMel

    return {log: LogMel(sample_rate, n_fft, hop, n_mels, log=log, **kw) for log in (None, "ln", "log10")}


def run_kernel(torch, ctx, x, spec, slack=37):
    """The call over x [rows, C, L] (numpy float32), stored with `slack` NaNs behind every plane, into an output prefilled
    with NaN that has GUARD elements of 0x5A bytes on both sides; returns (out [rows, C, n_mels, T'] numpy, guards intact)"""
    dev = torch.device("cuda", 0)
    rows, C_, L = x.shape
    Tf = spec.frames(L)
    src = np.full((rows, C_, L + slack), np.nan, dtype=np.float32)
    src[:, :, :L] = x
    n = rows * C_ * spec.n_mels * Tf
    raw = torch.full(((n + 2 * GUARD) * 4,), 0x5A, dtype=torch.uint8, device=dev).view(torch.float32)
    out = raw[GUARD:GUARD + n]
    out.fill_(float("nan"))
    window, basis, fb = spec.device_tables(dev)
    ctx.logmel_device(torch.from_numpy(src).to(dev), rows, C_, L + slack, L, spec.n_fft, spec.hop_length, spec.n_mels, window, basis,
                      fb, spec.log_mode, spec.floor, out, Tf, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    intact = bool((torch.cat([raw[:GUARD], raw[GUARD + n:]]).view(torch.uint8) == 0x5A).all())
    return out.cpu().numpy().reshape(rows, C_, spec.n_mels, Tf), intact


def check_power(got, x, spec, tag, twin=False):
    """|got - M| <= dM, every element; twin=True (full-scale noise): max |got - M| / dM is at most 4 times what the float32
    twin of the specification has on the same input"""
    from alac.net_amd.features import logmel_host, logmel_host_f32

    assert spec.log is None
    M, dM = logmel_host(x, spec, bound=True)
    assert got.shape == M.shape, (tag, got.shape, M.shape)
    assert np.isfinite(got).all(), (tag, "an element was not written, or is not finite")
    err = np.abs(got.astype(np.float64) - M)
    print(f"{tag}: max M {M.max():.3e}, max err {err.max():.3e}, max err / dM {np.max(err / np.maximum(dM, 1e-300)):.3f}")
    assert (err <= dM).all(), (tag, int(np.argmax(err - dM)), float(err.max()))
    if twin:
        r_gpu = float(np.max(err / np.maximum(dM, 1e-300)))
        r_ref = float(np.max(np.abs(logmel_host_f32(x, spec).astype(np.float64) - M) / np.maximum(dM, 1e-300)))
        print(f"{tag}: r_gpu {r_gpu:.5f}, r_ref {r_ref:.5f}, r_gpu / r_ref {r_gpu / r_ref:.3f}")
        assert r_gpu <= 4 * r_ref, (tag, r_gpu, r_ref)
    return M, dM


def check_log(got, M, dM, spec, tag):
    """got inside the log of [M - dM, M + dM], with logf's allowance; the input must be one whose interval is narrow"""
    assert spec.log in ("ln", "log10")
    fn = np.log if spec.log == "ln" else np.log10
    floor = float(np.float32(spec.floor))
    assert (M > 0).all() and (dM / M).max() <= 0.1, (tag, float((dM / np.maximum(M, 1e-300)).max()))
    lo, hi = fn(np.maximum(M - dM, floor)), fn(np.maximum(M + dM, floor))
    lo, hi = lo - 4 * U * (np.abs(lo) + 1), hi + 4 * U * (np.abs(hi) + 1)
    assert np.isfinite(got).all(), (tag, "an element was not written, or is not finite")
    g = got.astype(np.float64)
    want = fn(np.maximum(M, floor))
    print(f"{tag} {spec.log}: max dM / M {(dM / M).max():.3e}, max |got - log M| {np.abs(g - want).max():.3e}, "
          f"widest interval {(hi - lo).max():.3e}")
    assert ((g >= lo) & (g <= hi)).all(), (tag, spec.log, int(np.argmax(np.maximum(lo - g, g - hi))))


def check_log_any(got, M, dM, spec, tag):
    """got inside [log(max(M - dM, floor)) - e, log(max(M + dM, floor)) + e], e as in check_log, for any input.  Where
    M + dM < floor (M = 0 and M < 0 among them) every float32 evaluation is below the floor: those elements are logf(floor),
    one value inside e of log(floor), equal to one another bit for bit.  Not vacuous: at least 90 % of the elements are pinned
    in that way or have dM / M <= 0.1."""
    assert spec.log in ("ln", "log10")
    fn = np.log if spec.log == "ln" else np.log10
    floor = float(np.float32(spec.floor))
    pinned = M + dM < floor
    narrow = (M > 0) & (dM <= 0.1 * np.abs(M))
    assert (pinned | narrow).mean() >= 0.9, (tag, float((pinned | narrow).mean()))
    lo, hi = fn(np.maximum(M - dM, floor)), fn(np.maximum(M + dM, floor))
    lo, hi = lo - 4 * U * (np.abs(lo) + 1), hi + 4 * U * (np.abs(hi) + 1)
    assert got.shape == M.shape and np.isfinite(got).all(), (tag, "an element was not written, or is not finite")
    g = got.astype(np.float64)
    print(f"{tag} {spec.log} floor {floor:.3e}: {int(pinned.sum())} of {pinned.size} pinned to the floor, "
          f"{int((narrow & ~pinned).sum())} with dM / M <= 0.1, widest interval {(hi - lo).max():.3e}")
    assert ((g >= lo) & (g <= hi)).all(), (tag, spec.log, int(np.argmax(np.maximum(lo - g, g - hi))))
    if pinned.any():
        at = got[pinned]
        assert (at.view(np.int32) == at.view(np.int32).flat[0]).all(), (tag, spec.log, "the floor's log is not one value")
    return pinned


def noise(rng, *shape):
    return rng.uniform(-1.0, 1.0, shape).astype(np.float32)


@pytest.fixture(scope="module")
def gpu():
    import torch

    import alac.net_amd as pkg

    with pkg.AlacGpuContext([(4096, 16, 40, 10, 14, 2)]) as ctx:
        yield torch, pkg, ctx


@pytest.mark.parametrize("n_fft,hop,n_mels,L", SHAPES)
def test_kernel_equals_its_specification(gpu, n_fft, hop, n_mels, L):
    torch, pkg, ctx = gpu
    sp = specs(n_fft, hop, n_mels)
    rng = np.random.default_rng(n_fft)
    for channels in ((1, 2) if n_fft == 400 else (1,)):
        x = noise(rng, 2, channels, L)
        tag = f"({n_fft},{hop},{n_mels}) L {L} x{channels}"
        got, intact = run_kernel(torch, ctx, x, sp[None])
        assert intact, tag
        M, dM = check_power(got, x, sp[None], tag, twin=True)
        for log in ("ln", "log10"):
            got, intact = run_kernel(torch, ctx, x, sp[log])
            assert intact, (tag, log)
            check_log(got, M, dM, sp[log], tag)


def test_frame_counts_around_the_tile(gpu):
    """T' of 1, tile - 1, tile and tile + 1: a lone frame, a tile one short, a full one, and one frame in a tile of its own --
    for the tile of 32 and for a tile the span limit cuts down (n_fft = hop = 2048)"""
    torch, pkg, ctx = gpu
    rng = np.random.default_rng(7)
    tile = header_constant("ALAC_FEATURES_TILE")
    assert kernel_tile(400, 160) == tile and kernel_tile(2048, 512) == tile
    small = kernel_tile(2048, 2048)
    assert 1 < small < tile
    cases = [(16, 16, 4, 12)]                                                      # T' = 1 needs hop > n_fft // 2
    cases += [(400, 160, 80, 160 * (T - 1) + 5) for T in (tile - 1, tile, tile + 1)]
    cases += [(2048, 2048, 16, 2048 * (T - 1) + 1500) for T in (small - 1, small, small + 1)]
    for n_fft, hop, n_mels, L in cases:
        sp = specs(n_fft, hop, n_mels)[None]
        x = noise(rng, 1, 1, L)
        got, intact = run_kernel(torch, ctx, x, sp)
        assert intact and got.shape[-1] == 1 + L // hop
        check_power(got, x, sp, f"({n_fft},{hop},{n_mels}) T' {1 + L // hop}")


@pytest.mark.parametrize("n_fft,hop,n_mels", [(400, 160, 80), (25, 10, 8), (16, 1, 4), (25, 13, 8)])
def test_shortest_row_reflects_at_both_ends(gpu, n_fft, hop, n_mels):
    """L = n_fft // 2 + 1: a frame reflects at the front and at the back.  (25, 13): the last frame is centred on L and its last
    tap is the one a single reflection does not bring inside: it counts as zero"""
    torch, pkg, ctx = gpu
    from alac.net_amd.features import frame_index

    L = n_fft // 2 + 1
    idx, inside = frame_index(L, n_fft, hop)
    assert inside.all() == ((n_fft, hop) != (25, 13))
    sp = specs(n_fft, hop, n_mels)[None]
    x = noise(np.random.default_rng(L), 2, 1, L)
    got, intact = run_kernel(torch, ctx, x, sp)
    assert intact
    check_power(got, x, sp, f"({n_fft},{hop},{n_mels}) L {L}")


def test_tone_impulses_silence_and_tiny_input(gpu):
    torch, pkg, ctx = gpu
    n_fft, hop, n_mels, L = 400, 160, 80, 5000
    sp = specs(n_fft, hop, n_mels)
    n = np.arange(L, dtype=np.float64)
    tone = np.sin(2 * np.pi * 40 * n / n_fft)                    # on the centre of bin 40
    first, last = np.zeros(L), np.zeros(L)
    first[0] = last[L - 1] = 1.0
    tiny = np.random.default_rng(3).uniform(-1e-7, 1e-7, L)
    x = np.stack([tone, first, last, np.zeros(L), tiny]).astype(np.float32)[:, None, :]
    got, intact = run_kernel(torch, ctx, x, sp[None])
    assert intact
    M, _ = check_power(got, x, sp[None], "tone, impulses, silence, 1e-7")
    # (the tone's bin has power (sum of the window / 2)^2 = 1e4, times a filter weight of the order of 2 / (its width in Hz))
    assert M[0].max() > 10.0 and (got[3] == 0).all() and M[4].max() < 1e-10
    # silence: M = 0 and dM = 0, so every element is logf(floor), one value, inside logf's allowance around log(floor)
    for log, fn in (("ln", np.log), ("log10", np.log10)):
        got, intact = run_kernel(torch, ctx, x[3:4], sp[log])
        want = fn(float(np.float32(sp[log].floor)))
        print(f"silence {log}: {got.flat[0]!r} for {want!r}")
        assert intact and (got == got.flat[0]).all()
        assert abs(float(got.flat[0]) - want) <= 4 * U * (abs(want) + 1)


def test_callers_filterbank_is_used(gpu):
    torch, pkg, ctx = gpu
    from alac.net_amd.features import LogMel

    rng = np.random.default_rng(11)
    fb = rng.uniform(0.0, 1.0, (5, 201)).astype(np.float32)
    fb[2] = 0.0
    fb[3, :] = 0.0
    fb[3, 17] = 1.0                                              # one bin's power
    sp = LogMel(16000, 400, 160, filterbank=fb, log=None)
    assert sp.n_mels == 5 and np.array_equal(sp.fb, fb)
    x = noise(rng, 1, 1, 3000)
    got, intact = run_kernel(torch, ctx, x, sp)
    assert intact and (got[0, 0, 2] == 0).all()
    check_power(got, x, sp, "caller's filterbank")


def test_log_mel_on_tensors_and_lengths(gpu):
    """The public call: [F, C, T] as load_batch returns it, and lengths // hop + 1 with -1 kept"""
    torch, pkg, ctx = gpu
    sp = specs(400, 160, 80)
    x = noise(np.random.default_rng(5), 3, 2, 2000)
    d_x = torch.from_numpy(x).cuda()
    feats, lens = pkg.log_mel(d_x, sp[None], lengths=[2000, 161, -1])
    assert feats.shape == (3, 2, 80, 13) and feats.dtype == torch.float32 and lens.dtype == torch.int64
    assert lens.tolist() == [13, 2, -1]
    check_power(feats.cpu().numpy(), x, sp[None], "log_mel [F, C, T]")
    lens = pkg.log_mel(d_x, sp[None], lengths=torch.tensor([159, 160, -1], device="cuda"))[1]
    assert lens.is_cuda and lens.tolist() == [1, 2, -1]
    one = pkg.log_mel(d_x[1, 0], sp["ln"])
    assert one.shape == (80, 13)
    assert torch.equal(one, pkg.log_mel(d_x, sp["ln"])[1, 0])
    with pytest.raises(ValueError):
        pkg.log_mel(d_x[..., :200], sp[None])
    with pytest.raises(ValueError):
        pkg.log_mel(d_x.to(torch.float64), sp[None])


def test_two_streams_give_identical_bits(gpu):
    torch, pkg, ctx = gpu
    sp = specs(400, 160, 80)["ln"]
    d_x = torch.from_numpy(noise(np.random.default_rng(9), 8, 1, 8000)).cuda()
    torch.cuda.synchronize()
    outs = []
    for _ in range(2):
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            outs.append(pkg.log_mel(d_x, sp))
    torch.cuda.synchronize()
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))


def test_bad_arguments_return_before_any_enqueue(gpu):
    torch, pkg, ctx = gpu
    sp = specs(400, 160, 80)["ln"]
    dev = torch.device("cuda", 0)
    L, Tf = 1000, 7
    src = torch.zeros(L + 1, dtype=torch.float32, device=dev)
    out = torch.full((80 * Tf + 1,), 7.0, dtype=torch.float32, device=dev)
    window, basis, fb = sp.device_tables(dev)
    p = lambda t, off=0: t.data_ptr() + off
    good = dict(src=p(src), rows=1, channels=1, stride=L, frames=L, n_fft=400, hop=160, n_mels=80, window=p(window), basis=p(basis),
                fb=p(fb), log=1, floor=1e-10, out=p(out), out_frames=Tf)
    bad = [dict(src=None), dict(window=None), dict(basis=None), dict(fb=None), dict(out=None),
           dict(src=p(src, 2)), dict(window=p(window, 1)), dict(basis=p(basis, 2)), dict(fb=p(fb, 3)), dict(out=p(out, 2)),
           dict(n_fft=15), dict(n_fft=2049), dict(hop=0), dict(hop=401), dict(n_mels=0), dict(n_mels=257),
           dict(floor=0.0), dict(floor=-1.0), dict(floor=float("inf")), dict(floor=float("nan")), dict(log=3), dict(log=-1),
           dict(frames=200, out_frames=2), dict(out_frames=Tf + 1), dict(out_frames=Tf - 1), dict(channels=0),
           dict(frames=L + 1, out_frames=Tf),                                           # more signal than the stride holds
           dict(rows=1 << 31, frames=1 << 40, stride=1 << 40, out_frames=1 + (1 << 40) // 160)]   # 2^31 workgroups and more
    call = lambda a: pkg.lib().alacgpu_logmel_device(ctx._ctx, a["src"], a["rows"], a["channels"], a["stride"], a["frames"], a["n_fft"],
                                                     a["hop"], a["n_mels"], a["window"], a["basis"], a["fb"], a["log"], a["floor"],
                                                     a["out"], a["out_frames"], None)
    for change in bad:
        assert call({**good, **change}) == -1, change
    assert pkg.lib().alacgpu_logmel_device(None, *[good[k] for k in list(good)[:]], None) == -1
    torch.cuda.synchronize()
    assert (out == 7.0).all()
    assert call({**good, "rows": 0}) == 0                      # nothing happens
    torch.cuda.synchronize()
    assert (out == 7.0).all()
    assert call(good) == 0
    torch.cuda.synchronize()
    assert (out[:80 * Tf] != 7.0).all() and out[80 * Tf] == 7.0
