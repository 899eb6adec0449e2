"""alacgpu_fbank_device on the GPU against its specification in numpy (fbank.fbank_host), element by element.  The tolerance is
the derived one of fbank.py (its module docstring states it): in the power domain |got - M| <= dM, and on full-scale noise
max |got - M| / dM is at most 4 times what the float32 twin of the specification (fbank.fbank_host_f32: the kernel's arithmetic
one float32 operation at a time on the CPU) has on the same input -- the yardstick is the reference's own error, never the
kernel's.  With the log, got must lie in [ln(max(M - dM, floor)) - e, ln(max(M + dM, floor)) + e], e = 4 u (|ln| + 1) for logf;
pre-emphasis leaves the lowest filters little power, so that interval is wide for a few elements: the check is held from being
vacuous by a cap, at least 90 % of the elements have dM <= 0.1 M or are pinned below the floor (tests/test_fbank_spec.py
asserts the same on the CPU).  As in tests/test_features.py every plane has NaNs behind its signal and the output is prefilled
with NaN between guards of 0x5A bytes."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
GUARD = 64
# (win, hop, round_to_power_of_two, n_mels, L)
GRID = [(400, 160, True, 80, 5000), (25, 10, True, 8, 333), (16, 1, True, 4, 40), (512, 128, True, 64, 4000),
        (400, 160, False, 80, 5000), (2048, 512, True, 40, 9000)]
_SPEC_CACHE = {}


def spec_of(win=400, hop=160, n_mels=80, **kw):
    from alac.net_amd.fbank import KaldiFbank

    key = (win, hop, n_mels, tuple(sorted(kw.items())))
    if key not in _SPEC_CACHE:
        _SPEC_CACHE[key] = KaldiFbank(16000, win, hop, n_mels, **kw)
    return _SPEC_CACHE[key]


def run_kernel(torch, ctx, x, spec, slack=37, stream=None):
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
    ctx.fbank_device(torch.from_numpy(src).to(dev), rows, C_, L + slack, L, spec.win_length, spec.n_fft, spec.hop_length, spec.n_mels,
                     window, basis, fb, spec.flags, spec.preemphasis, spec.scale, raw[GUARD:], Tf,
                     stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    intact = bool((torch.cat([raw[:GUARD], raw[GUARD + n:]]).view(torch.uint8) == 0x5A).all())
    return out.cpu().numpy().reshape(rows, C_, spec.n_mels, Tf), intact


def check_power(got, x, spec, tag, twin=False):
    """|got - M| <= dM, every element; twin=True (full-scale noise): max |got - M| / dM is at most 4 times the twin's"""
    from alac.net_amd.fbank import fbank_host, fbank_host_f32

    assert not spec.log
    M, dM = fbank_host(x, spec, bound=True)
    assert got.shape == M.shape, (tag, got.shape, M.shape)
    assert np.isfinite(got).all(), (tag, "an element was not written, or is not finite")
    err = np.abs(got.astype(np.float64) - M)
    print(f"{tag}: max M {M.max():.3e}, max err {err.max():.3e}, max err / dM {np.max(err / np.maximum(dM, 1e-300)):.4f}")
    assert (err <= dM).all(), (tag, int(np.argmax(err - dM)), float(err.max()))
    if twin:
        r_gpu = float(np.max(err / np.maximum(dM, 1e-300)))
        r_ref = float(np.max(np.abs(fbank_host_f32(x, spec).astype(np.float64) - M) / np.maximum(dM, 1e-300)))
        print(f"{tag}: r_gpu {r_gpu:.5f}, r_ref {r_ref:.5f}, r_gpu / r_ref {r_gpu / r_ref:.3f}")
        assert r_gpu <= 4 * r_ref, (tag, r_gpu, r_ref)
    return M, dM


def check_log(got, M, dM, tag):
    """got inside [ln(max(M - dM, floor)) - e, ln(max(M + dM, floor)) + e] with e = 4 u (|ln| + 1); at least 90 % of the
    elements are pinned below the floor or have dM <= 0.1 M"""
    from alac.net_amd.fbank import FLOOR

    pinned = M + dM < FLOOR
    narrow = (M > 0) & (dM <= 0.1 * np.abs(M))
    assert (pinned | narrow).mean() >= 0.9, (tag, float((pinned | narrow).mean()))
    lo, hi = np.log(np.maximum(M - dM, FLOOR)), np.log(np.maximum(M + dM, FLOOR))
    lo, hi = lo - 4 * U * (np.abs(lo) + 1), hi + 4 * U * (np.abs(hi) + 1)
    assert got.shape == M.shape and np.isfinite(got).all(), (tag, "an element was not written, or is not finite")
    g = got.astype(np.float64)
    print(f"{tag} ln: {int(pinned.sum())} of {pinned.size} pinned, {int((narrow & ~pinned).sum())} with dM <= 0.1 M, "
          f"max |got - ln M| {np.abs(g - np.log(np.maximum(M, FLOOR))).max():.3e}, widest interval {(hi - lo).max():.3e}")
    assert ((g >= lo) & (g <= hi)).all(), (tag, int(np.argmax(np.maximum(lo - g, g - hi))))


def noise(rng, *shape):
    return rng.uniform(-1.0, 1.0, shape).astype(np.float32)


@pytest.fixture(scope="module")
def gpu():
    import torch

    import alac.net_amd as pkg

    with pkg.AlacGpuContext([(4096, 16, 40, 10, 14, 2)]) as ctx:
        yield torch, pkg, ctx


@pytest.mark.parametrize("snip", [True, False])
@pytest.mark.parametrize("win,hop,pow2,n_mels,L", GRID)
def test_kernel_equals_its_specification(gpu, win, hop, pow2, n_mels, L, snip):
    torch, pkg, ctx = gpu
    power = spec_of(win, hop, n_mels, round_to_power_of_two=pow2, snip_edges=snip, log=False)
    logged = spec_of(win, hop, n_mels, round_to_power_of_two=pow2, snip_edges=snip)
    rng = np.random.default_rng(win)
    for channels in ((1, 2) if (win, pow2) == (400, True) else (1,)):
        x = noise(rng, 1 if win == 2048 else 2, channels, L)
        tag = f"({win},{hop},{power.n_fft},{n_mels}) L {L} x{channels} snip {snip}"
        got, intact = run_kernel(torch, ctx, x, power)
        assert intact, tag
        M, dM = check_power(got, x, power, tag, twin=True)
        got, intact = run_kernel(torch, ctx, x, logged)
        assert intact, tag
        check_log(got, M, dM, tag)


@pytest.mark.parametrize("snip", [True, False])
def test_frame_counts_around_the_tile(gpu, snip):
    """T' of 1, 31, 32, 33, 64 and 65 at hop 160: a lone frame, a tile one short, full tiles, one frame in a tile of its own"""
    torch, pkg, ctx = gpu
    spec = spec_of(snip_edges=snip, log=False)
    rng = np.random.default_rng(7)
    for T in (1, 31, 32, 33, 64, 65):
        L = 400 + 160 * (T - 1) + 5 if snip else 160 * T - 80 + 3
        assert spec.frames(L) == T
        x = noise(rng, 1, 1, L)
        got, intact = run_kernel(torch, ctx, x, spec)
        assert intact and got.shape[-1] == T                     # (check_power: every element was written)
        check_power(got, x, spec, f"T' {T} snip {snip}")


def test_short_and_edge_rows(gpu):
    torch, pkg, ctx = gpu
    rng = np.random.default_rng(8)
    for snip in (True, False):                                    # L = win: exactly one frame with snip_edges
        spec = spec_of(snip_edges=snip, log=False)
        x = noise(rng, 2, 1, 400)
        got, intact = run_kernel(torch, ctx, x, spec)
        assert intact and got.shape[-1] == (1 if snip else 3)       # (400 + 80) // 160
        check_power(got, x, spec, f"L = win snip {snip}")
    # L = win - 1 with snip_edges: no frame, no launch, nothing written
    spec = spec_of(log=False)
    got, intact = run_kernel(torch, ctx, noise(rng, 2, 1, 399), spec)
    assert intact and got.shape == (2, 1, 80, 0)
    assert pkg.fbank(torch.zeros(3, 399, device="cuda"), spec).shape == (3, 80, 0)
    # L = 5 under a window of 25: the repeated reflection; and a row of one sample
    for win, hop, L in ((25, 10, 5), (25, 10, 1), (16, 1, 3), (400, 160, 100)):
        spec = spec_of(win, hop, 8, snip_edges=False, log=False)
        x = noise(rng, 2, 1, L) + np.float32(0.5)
        got, intact = run_kernel(torch, ctx, x, spec)
        assert intact and got.shape[-1] == (L + hop // 2) // hop
        if got.shape[-1]:
            check_power(got, x, spec, f"({win},{hop}) L {L} reflected")


@pytest.mark.parametrize("kw", [dict(remove_dc_offset=False), dict(preemphasis=0.0), dict(use_power=False), dict(scale=1.0),
                                dict(window="hamming")], ids=lambda kw: next(iter(kw)))
def test_each_switch_alone(gpu, kw):
    torch, pkg, ctx = gpu
    rng = np.random.default_rng(9)
    x = noise(rng, 2, 1, 3000) + np.float32(0.1)                  # an offset for remove_dc_offset to matter
    power, default = spec_of(log=False, **kw), spec_of(log=False)
    got, intact = run_kernel(torch, ctx, x, power)
    assert intact
    M, dM = check_power(got, x, power, str(kw), twin=True)
    base, _ = run_kernel(torch, ctx, x, default)
    assert not np.array_equal(base, got), kw                       # the switch does something
    got, intact = run_kernel(torch, ctx, x, spec_of(**kw))
    assert intact
    check_log(got, M, dM, str(kw))


def test_constant_silence_and_a_nan(gpu):
    torch, pkg, ctx = gpu
    from alac.net_amd.fbank import FLOOR, fbank_frame_index

    power, logged = spec_of(log=False), spec_of()
    L = 3000
    const = np.stack([np.full(L, 0.3), np.full(L, 0.25), np.zeros(L)]).astype(np.float32)[:, None, :]
    got, intact = run_kernel(torch, ctx, const, power)
    assert intact
    check_power(got, const, power, "constants and silence")
    assert (got[1:] == 0).all()                                   # 8192 and its sums are exact: the mean is the constant
    got, intact = run_kernel(torch, ctx, const[2:], logged)
    want = np.log(FLOOR)
    print(f"silence: {got.flat[0]!r} for {want!r}")
    assert intact and (got.view(np.int32) == got.view(np.int32).flat[0]).all()
    assert abs(float(got.flat[0]) - want) <= 4 * U * (abs(want) + 1)
    # a NaN at one sample reaches exactly the frames that contain it; every other frame is bit for bit the run without it
    rng = np.random.default_rng(10)
    x = noise(rng, 2, 1, 5000)
    y = x.copy()
    y[1, 0, 1700] = np.nan
    for snip in (True, False):
        for kw in (dict(), dict(remove_dc_offset=False)):
            spec = spec_of(snip_edges=snip, **kw)
            hit = (fbank_frame_index(5000, spec) == 1700).any(axis=1)
            clean, _ = run_kernel(torch, ctx, x, spec)
            dirty, intact = run_kernel(torch, ctx, y, spec)
            assert intact and 1 < hit.sum() < 4
            assert np.isnan(dirty[1, 0][:, hit]).all()
            assert np.array_equal(dirty[1, 0][:, ~hit].view(np.int32), clean[1, 0][:, ~hit].view(np.int32))
            assert np.array_equal(dirty[0].view(np.int32), clean[0].view(np.int32))


def test_fbank_on_tensors_and_lengths(gpu):
    torch, pkg, ctx = gpu
    spec = spec_of(log=False)
    x = noise(np.random.default_rng(5), 3, 2, 2000)
    d_x = torch.from_numpy(x).cuda()
    feats, lens = pkg.fbank(d_x, spec, lengths=[2000, 400, -1])
    assert feats.shape == (3, 2, 80, 11) and feats.dtype == torch.float32 and lens.dtype == torch.int64
    assert lens.tolist() == [11, 1, -1]
    check_power(feats.cpu().numpy(), x, spec, "fbank [F, C, T]")
    lens = pkg.fbank(d_x, spec, lengths=torch.tensor([399, 560, -1], device="cuda"))[1]
    assert lens.is_cuda and lens.tolist() == [0, 2, -1]
    one = pkg.fbank(d_x[1, 0], spec_of())
    assert one.shape == (80, 11) and torch.equal(one, pkg.fbank(d_x, spec_of())[1, 0])
    for bad in (lambda: pkg.fbank(d_x.to(torch.float64), spec), lambda: pkg.fbank(d_x.cpu(), spec), lambda: pkg.fbank(d_x, pkg.LogMel(16000)),
                lambda: pkg.fbank(d_x[..., :0], spec), lambda: pkg.log_mel(d_x, spec)):
        with pytest.raises(ValueError):
            bad()


def test_two_streams_give_identical_bits(gpu):
    torch, pkg, ctx = gpu
    spec = spec_of()
    d_x = torch.from_numpy(noise(np.random.default_rng(9), 8, 1, 8000)).cuda()
    torch.cuda.synchronize()
    outs = []
    for _ in range(2):
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            outs.append(pkg.fbank(d_x, spec))
    torch.cuda.synchronize()
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))


def test_bad_arguments_return_before_any_enqueue(gpu):
    torch, pkg, ctx = gpu
    spec = spec_of()
    dev = torch.device("cuda", 0)
    L, Tf = 1000, 4
    src = torch.zeros(L + 1, dtype=torch.float32, device=dev)
    out = torch.full((80 * Tf + 1,), 7.0, dtype=torch.float32, device=dev)
    window, basis, fb = spec.device_tables(dev)
    p = lambda t, off=0: t.data_ptr() + off
    good = dict(src=p(src), rows=1, channels=1, stride=L, frames=L, win=400, n_fft=512, hop=160, n_mels=80, window=p(window),
                basis=p(basis), fb=p(fb), flags=15, pre=0.97, scale=32768.0, out=p(out), out_frames=Tf)
    bad = [dict(src=None), dict(window=None), dict(basis=None), dict(fb=None), dict(out=None),
           dict(src=p(src, 2)), dict(window=p(window, 1)), dict(basis=p(basis, 2)), dict(fb=p(fb, 3)), dict(out=p(out, 2)),
           dict(win=15), dict(win=2049, n_fft=2049), dict(n_fft=399), dict(n_fft=2049), dict(hop=0), dict(hop=401), dict(n_mels=0),
           dict(n_mels=257), dict(flags=16), dict(pre=-0.5), dict(pre=1.5), dict(pre=float("nan")), dict(scale=0.0),
           dict(scale=float("inf")), dict(scale=float("nan")), dict(channels=0), dict(frames=0, out_frames=0),
           dict(out_frames=Tf + 1), dict(out_frames=Tf - 1), dict(flags=14, out_frames=Tf),        # centred: 6 frames
           dict(frames=L + 1, out_frames=Tf),                                                     # more signal than the stride holds
           dict(rows=1 << 31, frames=1 << 40, stride=1 << 40, out_frames=1 + ((1 << 40) - 400) // 160)]   # 2^31 workgroups and more
    call = lambda a: pkg.lib().alacgpu_fbank_device(ctx._ctx, a["src"], a["rows"], a["channels"], a["stride"], a["frames"], a["win"],
                                                    a["n_fft"], a["hop"], a["n_mels"], a["window"], a["basis"], a["fb"], a["flags"],
                                                    a["pre"], a["scale"], a["out"], a["out_frames"], None)
    for change in bad:
        assert call({**good, **change}) == -1, change
    assert pkg.lib().alacgpu_fbank_device(None, *[good[k] for k in good], None) == -1
    torch.cuda.synchronize()
    assert (out == 7.0).all()
    assert call({**good, "rows": 0}) == 0                      # nothing happens
    assert call({**good, "frames": 399, "out_frames": 0}) == 0  # no frame: nothing happens
    torch.cuda.synchronize()
    assert (out == 7.0).all()
    assert call(good) == 0
    torch.cuda.synchronize()
    assert (out[:80 * Tf] != 7.0).all() and out[80 * Tf] == 7.0
