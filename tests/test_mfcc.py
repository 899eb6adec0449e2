"""alacgpu_mfcc_device on the GPU against its specification in numpy (mfcc.mfcc_host), element by element, in the harness of
tests/test_fbank.py: NaNs behind every plane, the output prefilled with NaN between guards of 0x5A bytes.  Two yardsticks.
The derived bound of mfcc.py: |got - out| <= dC, and max |got - out| / dC is at most 4 times what the float32 twin
(mfcc.mfcc_host_f32) has on the same input -- the reference's own error, never the kernel's; tests/test_mfcc_spec.py holds dC
from being vacuous (dC <= 1 where the median of |out| is above 3).  And the tight one, which needs no cap: the cepstra are the
DCT of the fbank kernel's own bits -- with F the float32 output of alacgpu_fbank_device (log) on the same input and tables,
got[c] lies within lifter_c (n_mels + 1) u sum |dct[c, m] F[m]| + u |got[c]| of lifter_c sum dct[c, m] F[m] in float64 --
which catches any reordering or re-flooring in the epilogue."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
GUARD = 64
LN_FLOOR = float(np.log(2.0 ** -23))
# (win, hop, filters, cepstra, L, the snip_edges of the issue's CPU figures); both values of snip_edges run
GRID = [(400, 160, 23, 13, 5000), (400, 160, 80, 80, 5000), (25, 10, 8, 5, 333), (16, 1, 4, 4, 40), (2048, 512, 40, 20, 9000)]
_SPEC_CACHE = {}


def spec_of(win=400, hop=160, n_mels=23, n_ceps=13, **kw):
    from alac.net_amd.mfcc import KaldiMfcc

    key = (win, hop, n_mels, n_ceps, tuple(sorted(kw.items())))
    if key not in _SPEC_CACHE:
        _SPEC_CACHE[key] = KaldiMfcc(16000, win, hop, n_mels, n_ceps, **kw)
    return _SPEC_CACHE[key]


def fbank_of(spec):
    """The KaldiFbank with the tables and switches of a KaldiMfcc, logged"""
    from alac.net_amd.fbank import KaldiFbank

    key = ("fbank", id(spec))
    if key not in _SPEC_CACHE:
        _SPEC_CACHE[key] = KaldiFbank(16000, spec.win_length, spec.hop_length, spec.n_filters, spec.low_freq, spec.high_freq,
                                      spec.preemphasis, spec.remove_dc_offset, spec.window_type, spec.round_to_power_of_two,
                                      spec.snip_edges, spec.use_power, True, spec.scale)
    return _SPEC_CACHE[key]


def guarded(torch, n):
    raw = torch.full(((n + 2 * GUARD) * 4,), 0x5A, dtype=torch.uint8, device="cuda").view(torch.float32)
    raw[GUARD:GUARD + n].fill_(float("nan"))
    return raw, lambda: bool((torch.cat([raw[:GUARD], raw[GUARD + n:]]).view(torch.uint8) == 0x5A).all())


def run_kernel(torch, ctx, x, spec, slack=37, fbank=False):
    """The call over x [rows, C, L] (numpy float32), stored with `slack` NaNs behind every plane, into an output prefilled
    with NaN that has GUARD elements of 0x5A bytes on both sides; returns (out [rows, C, n_ceps, T'] numpy, guards intact).
    fbank=True: alacgpu_fbank_device with log on the same input and the same three tables, [rows, C, n_filters, T']."""
    dev = torch.device("cuda", 0)
    rows, C_, L = x.shape
    Tf = spec.frames(L)
    src = np.full((rows, C_, L + slack), np.nan, dtype=np.float32)
    src[:, :, :L] = x
    lines = spec.n_filters if fbank else spec.n_ceps
    n = rows * C_ * lines * Tf
    raw, intact = guarded(torch, n)
    window, basis, fb, dct, lifter = spec.device_tables(dev)
    stream = torch.cuda.current_stream().cuda_stream
    if fbank:
        ctx.fbank_device(torch.from_numpy(src).to(dev), rows, C_, L + slack, L, spec.win_length, spec.n_fft, spec.hop_length,
                         spec.n_filters, window, basis, fb, fbank_of(spec).flags, spec.preemphasis, spec.scale, raw[GUARD:], Tf, stream=stream)
    else:
        ctx.mfcc_device(torch.from_numpy(src).to(dev), rows, C_, L + slack, L, spec.win_length, spec.n_fft, spec.hop_length,
                        spec.n_filters, spec.n_ceps, window, basis, fb, dct, lifter, spec.flags, spec.preemphasis, spec.scale,
                        spec.energy_floor, raw[GUARD:], Tf, stream=stream)
    torch.cuda.synchronize()
    return raw[GUARD:GUARD + n].cpu().numpy().reshape(rows, C_, lines, Tf), intact()


def check_bound(got, x, spec, tag, twin=False):
    """|got - out| <= dC, every element; twin=True (full-scale noise): max |got - out| / dC is at most 4 times the twin's"""
    from alac.net_amd.mfcc import mfcc_host, mfcc_host_f32

    out, dC = mfcc_host(x, spec, bound=True)
    assert got.shape == out.shape, (tag, got.shape, out.shape)
    assert np.isfinite(got).all(), (tag, "an element was not written, or is not finite")
    err = np.abs(got.astype(np.float64) - out)
    print(f"{tag}: max |out| {np.abs(out).max():.3f}, max err {err.max():.3e}, max err / dC {np.max(err / dC):.5f}")
    assert (err <= dC).all(), (tag, int(np.argmax(err - dC)), float(err.max()))
    if twin:
        r_gpu = float(np.max(err / dC))
        r_ref = float(np.max(np.abs(mfcc_host_f32(x, spec).astype(np.float64) - out) / dC))
        print(f"{tag}: r_gpu {r_gpu:.5f}, r_ref {r_ref:.5f}, r_gpu / r_ref {r_gpu / r_ref:.3f}")
        assert r_gpu <= 4 * r_ref, (tag, r_gpu, r_ref)
    return out, dC


def check_dct_of_fbank(got, F, spec, tag):
    """got[c] within |lifter_c| (n_mels + 1) u sum_m |dct[c, m] F[m]| + u |got[c]| of lifter_c sum_m dct[c, m] F[m], F the fbank
    kernel's float32 log-mel; with use_energy line 0 is not a cepstrum and is left out"""
    dct, lifter = spec.dct.astype(np.float64), spec.lifter.astype(np.float64)
    F = F.astype(np.float64)                                          # [rows, C, n_filters, T]
    want = lifter[:, None] * np.einsum("cm,rkmt->rkct", dct, F)
    tol = (np.abs(lifter)[:, None] * (spec.n_filters + 1) * U * np.einsum("cm,rkmt->rkct", np.abs(dct), np.abs(F))
           + U * np.abs(got.astype(np.float64)))
    err = np.abs(got.astype(np.float64) - want)
    first = 1 if spec.use_energy else 0
    print(f"{tag}: DCT of the fbank kernel's bits: max err {err[:, :, first:].max():.3e}, max err / tol "
          f"{np.max(err[:, :, first:] / tol[:, :, first:]):.4f}")
    assert (err <= tol)[:, :, first:].all(), (tag, float(np.max(err[:, :, first:] / tol[:, :, first:])))


def noise(rng, *shape):
    return rng.uniform(-1.0, 1.0, shape).astype(np.float32)


@pytest.fixture(scope="module")
def gpu():
    import torch

    import alac.net_amd as pkg

    with pkg.AlacGpuContext([(4096, 16, 40, 10, 14, 2)]) as ctx:
        yield torch, pkg, ctx


@pytest.mark.parametrize("snip", [True, False])
@pytest.mark.parametrize("win,hop,n_mels,n_ceps,L", GRID)
def test_kernel_equals_its_specification(gpu, win, hop, n_mels, n_ceps, L, snip):
    torch, pkg, ctx = gpu
    spec = spec_of(win, hop, n_mels, n_ceps, snip_edges=snip)
    rng = np.random.default_rng(win)
    for channels in ((1, 2) if (win, n_mels) == (400, 23) else (1,)):
        x = noise(rng, 1 if win == 2048 or n_mels == 80 else 2, channels, L)
        tag = f"({win},{hop},{n_mels},{n_ceps}) L {L} x{channels} snip {snip}"
        got, intact = run_kernel(torch, ctx, x, spec)
        assert intact, tag
        check_bound(got, x, spec, tag, twin=True)
        F, intact = run_kernel(torch, ctx, x, spec, fbank=True)
        assert intact, tag
        check_dct_of_fbank(got, F, spec, tag)


@pytest.mark.parametrize("snip", [True, False])
def test_frame_counts_around_the_tile(gpu, snip):
    """T' of 1, 31, 32, 33 and 65 at hop 160: a lone frame, a tile one short, a full tile, one frame in a tile of its own"""
    torch, pkg, ctx = gpu
    spec = spec_of(snip_edges=snip, use_energy=True)
    rng = np.random.default_rng(7)
    for T in (1, 31, 32, 33, 65):
        L = 400 + 160 * (T - 1) + 5 if snip else 160 * T - 80 + 3
        assert spec.frames(L) == T
        x = noise(rng, 1, 1, L)
        got, intact = run_kernel(torch, ctx, x, spec)
        assert intact and got.shape[-1] == T                       # (check_bound: every element was written)
        check_bound(got, x, spec, f"T' {T} snip {snip}")
        check_dct_of_fbank(got, run_kernel(torch, ctx, x, spec, fbank=True)[0], spec, f"T' {T} snip {snip}")


# (the switch, the transform it is switched on: the two must differ)
SWITCHES = [(dict(use_energy=True), dict()), (dict(use_energy=True, raw_energy=False), dict(use_energy=True)),
            (dict(use_energy=True, energy_floor=7e10), dict(use_energy=True)), (dict(cepstral_lifter=0.0), dict()),
            (dict(n_ceps=1), dict()), (dict(n_ceps=23), dict()), (dict(use_power=False), dict()),
            (dict(use_energy=True, remove_dc_offset=False), dict(remove_dc_offset=False)),
            (dict(use_energy=True, raw_energy=False, preemphasis=0.0), dict(use_energy=True, preemphasis=0.0))]


@pytest.mark.parametrize("kw,before", SWITCHES, ids=[",".join(f"{k}={v}" for k, v in kw.items()) for kw, _ in SWITCHES])
def test_each_switch_alone(gpu, kw, before):
    torch, pkg, ctx = gpu
    rng = np.random.default_rng(9)
    x = noise(rng, 2, 1, 3000) + np.float32(0.1)                  # an offset for remove_dc_offset to matter
    x[1] *= np.float32(0.5)                                       # (row 0's energies lie above the floor of 7e10, row 1's below)
    spec = spec_of(**kw)
    got, intact = run_kernel(torch, ctx, x, spec)
    assert intact
    out, dC = check_bound(got, x, spec, str(kw), twin=True)
    check_dct_of_fbank(got, run_kernel(torch, ctx, x, spec, fbank=True)[0], spec, str(kw))
    base, _ = run_kernel(torch, ctx, x, spec_of(**before))
    n = min(base.shape[2], got.shape[2])
    assert base.shape != got.shape or not np.array_equal(base, got), kw          # the switch does something
    if spec.use_energy:                                           # the energy is line 0 and nothing else
        assert not np.array_equal(base[:, :, 0], got[:, :, 0]), kw
        assert np.array_equal(base[:, :, 1:].view(np.int32), got[:, :, 1:].view(np.int32)), kw
    if spec.energy_floor:
        assert (got[1, 0, 0] == np.float32(spec.log_energy_floor)).all() and (got[0, 0, 0] > np.float32(spec.log_energy_floor)).all()
        assert np.array_equal(got[0], base[0])
    if spec.n_ceps != 13:                                         # fewer or more cepstra are the same lines
        assert np.array_equal(base[:, :, :n].view(np.int32), got[:, :, :n].view(np.int32)), kw


def test_silence_and_a_nan(gpu):
    torch, pkg, ctx = gpu
    from alac.net_amd.fbank import fbank_frame_index

    L = 3000
    z = np.zeros((1, 1, L), dtype=np.float32)
    for kw in (dict(), dict(use_energy=True), dict(use_energy=True, energy_floor=0.25)):
        spec = spec_of(**kw)
        got, intact = run_kernel(torch, ctx, z, spec)
        assert intact
        check_bound(got, z, spec, f"silence {kw}")
        want = spec.lifter.astype(np.float64) * LN_FLOOR * spec.dct.astype(np.float64).sum(axis=1)
        tol = np.abs(spec.lifter) * (4 * U * 17 * np.abs(spec.dct).sum(axis=1) + 24 * U * np.abs(spec.dct).sum(axis=1) * 16) + U * np.abs(want)
        first = 1 if spec.use_energy else 0
        assert (np.abs(got[0, 0].astype(np.float64) - want[:, None]) <= tol[:, None])[first:].all(), kw
        assert (got[0, 0].view(np.int32) == got[0, 0, :, :1].view(np.int32)).all()        # every frame the same bits
        if spec.use_energy:
            e = float(got[0, 0, 0, 0])
            print(f"silence {kw}: energy {e!r}")
            if spec.energy_floor:
                assert e == float(np.float32(np.log(0.25)))
            else:
                assert abs(e - LN_FLOOR) <= 4 * U * (abs(LN_FLOOR) + 1)
    # a NaN at one sample reaches exactly the frames that contain it, in every cepstrum; every other frame is bit for bit clean
    rng = np.random.default_rng(10)
    x = noise(rng, 2, 1, 5000)
    y = x.copy()
    y[1, 0, 1700] = np.nan
    for snip in (True, False):
        for kw in (dict(), dict(use_energy=True), dict(use_energy=True, raw_energy=False, energy_floor=1.0)):
            spec = spec_of(snip_edges=snip, **kw)
            hit = (fbank_frame_index(5000, spec) == 1700).any(axis=1)
            clean, _ = run_kernel(torch, ctx, x, spec)
            dirty, intact = run_kernel(torch, ctx, y, spec)
            assert intact and 1 < hit.sum() < 4
            assert np.isnan(dirty[1, 0][:, hit]).all(), (snip, kw)
            assert np.array_equal(dirty[1, 0][:, ~hit].view(np.int32), clean[1, 0][:, ~hit].view(np.int32))
            assert np.array_equal(dirty[0].view(np.int32), clean[0].view(np.int32))


def test_mfcc_on_tensors_and_lengths(gpu):
    torch, pkg, ctx = gpu
    spec = spec_of()
    x = noise(np.random.default_rng(5), 3, 2, 2000)
    d_x = torch.from_numpy(x).cuda()
    feats, lens = pkg.mfcc(d_x, spec, lengths=[2000, 400, -1])
    assert feats.shape == (3, 2, 13, 11) and feats.dtype == torch.float32 and lens.dtype == torch.int64
    assert lens.tolist() == [11, 1, -1]
    check_bound(feats.cpu().numpy(), x, spec, "mfcc [F, C, T]")
    lens = pkg.mfcc(d_x, spec, lengths=torch.tensor([399, 560, -1], device="cuda"))[1]
    assert lens.is_cuda and lens.tolist() == [0, 2, -1]
    one = pkg.mfcc(d_x[1, 0], spec)
    assert one.shape == (13, 11) and torch.equal(one, feats[1, 0])
    assert pkg.mfcc(torch.zeros(3, 399, device="cuda"), spec).shape == (3, 13, 0)
    for bad in (lambda: pkg.mfcc(d_x.to(torch.float64), spec), lambda: pkg.mfcc(d_x.cpu(), spec), lambda: pkg.mfcc(d_x, pkg.KaldiFbank(16000)),
                lambda: pkg.mfcc(d_x[..., :0], spec), lambda: pkg.fbank(d_x, spec)):
        with pytest.raises(ValueError):
            bad()


def test_two_streams_give_identical_bits(gpu):
    torch, pkg, ctx = gpu
    spec = spec_of(use_energy=True)
    d_x = torch.from_numpy(noise(np.random.default_rng(9), 8, 1, 8000)).cuda()
    torch.cuda.synchronize()
    outs = []
    for _ in range(2):
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            outs.append(pkg.mfcc(d_x, spec))
    torch.cuda.synchronize()
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))


def test_bad_arguments_return_before_any_enqueue(gpu):
    torch, pkg, ctx = gpu
    spec = spec_of()
    dev = torch.device("cuda", 0)
    L, Tf = 1000, 4
    src = torch.zeros(L + 1, dtype=torch.float32, device=dev)
    out = torch.full((13 * Tf + 1,), 7.0, dtype=torch.float32, device=dev)
    window, basis, fb, dct, lifter = spec.device_tables(dev)
    p = lambda t, off=0: t.data_ptr() + off
    good = dict(src=p(src), rows=1, channels=1, stride=L, frames=L, win=400, n_fft=512, hop=160, n_mels=23, n_ceps=13, window=p(window),
                basis=p(basis), fb=p(fb), dct=p(dct), lifter=p(lifter), flags=7, pre=0.97, scale=32768.0, floor=0.0, out=p(out),
                out_frames=Tf)
    bad = [dict(src=None), dict(window=None), dict(basis=None), dict(fb=None), dict(dct=None), dict(lifter=None), dict(out=None),
           dict(src=p(src, 2)), dict(window=p(window, 1)), dict(basis=p(basis, 2)), dict(fb=p(fb, 3)), dict(dct=p(dct, 2)),
           dict(lifter=p(lifter, 1)), dict(out=p(out, 2)),
           dict(win=15), dict(win=2049, n_fft=2049), dict(n_fft=399), dict(n_fft=2049), dict(hop=0), dict(hop=401), dict(n_mels=0),
           dict(n_mels=257), dict(n_ceps=0), dict(n_ceps=24), dict(flags=8 + 7), dict(flags=64 + 7), dict(flags=32 + 7), dict(flags=128),
           dict(pre=-0.5), dict(pre=1.5), dict(pre=float("nan")), dict(scale=0.0), dict(scale=float("inf")), dict(scale=float("nan")),
           dict(floor=-1.0), dict(floor=float("inf")), dict(floor=float("nan")), dict(channels=0), dict(frames=0, out_frames=0),
           dict(out_frames=Tf + 1), dict(out_frames=Tf - 1), dict(flags=6, out_frames=Tf),          # centred: 6 frames
           dict(frames=L + 1, out_frames=Tf),                                                     # more signal than the stride holds
           dict(rows=1 << 31, frames=1 << 40, stride=1 << 40, out_frames=1 + ((1 << 40) - 400) // 160)]   # 2^31 workgroups and more
    call = lambda a: pkg.lib().alacgpu_mfcc_device(ctx._ctx, a["src"], a["rows"], a["channels"], a["stride"], a["frames"], a["win"],
                                                   a["n_fft"], a["hop"], a["n_mels"], a["n_ceps"], a["window"], a["basis"], a["fb"],
                                                   a["dct"], a["lifter"], a["flags"], a["pre"], a["scale"], a["floor"], a["out"],
                                                   a["out_frames"], None)
    for change in bad:
        assert call({**good, **change}) == -1, change
    assert pkg.lib().alacgpu_mfcc_device(None, *[good[k] for k in good], None) == -1
    torch.cuda.synchronize()
    assert (out == 7.0).all()
    assert call({**good, "rows": 0}) == 0                      # nothing happens
    assert call({**good, "frames": 399, "out_frames": 0}) == 0  # no frame: nothing happens
    torch.cuda.synchronize()
    assert (out == 7.0).all()
    for flags in (7, 7 + 16, 7 + 16 + 32):
        out.fill_(7.0)
        assert call({**good, "flags": flags, "floor": 1.0}) == 0
        torch.cuda.synchronize()
        assert (out[:13 * Tf] != 7.0).all() and out[13 * Tf] == 7.0
