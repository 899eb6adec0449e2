"""alacgpu_logmel_device by code path: the grid of tests/test_features_spec.py (one shape per branch of alac_features.hip)
against the specification and its float32 twin, many tiles with every frame compared, properties that need no tolerance
(a frame does not depend on where it sits, nor a plane on its neighbours), the log and the floor on any input, and what
is not finite.  The checks are those of tests/test_features.py; `L` is small: the kernel's paths depend on n_fft, hop, n_mels
and the number of tiles, not on the length of the audio."""
import numpy as np
import pytest

from test_features import (GUARD, U, check_log_any, check_power, gpu, header_constant, kernel_tile, noise,  # noqa: F401
                           run_kernel, specs)
from test_features_spec import GRID

pytestmark = pytest.mark.gpu

TWO_CHANNELS = [(402, 161, 80, 3000), (18, 3, 5, 60)]


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


@pytest.mark.parametrize("n_fft,hop,n_mels,L", GRID)
def test_grid_equals_the_specification_and_its_twin(gpu, n_fft, hop, n_mels, L):
    torch, pkg, ctx = gpu
    assert set(TWO_CHANNELS) <= set(GRID)
    sp = specs(n_fft, hop, n_mels)
    rng = np.random.default_rng(n_fft)
    for channels in ((1, 2) if (n_fft, hop, n_mels, L) in TWO_CHANNELS else (1,)):
        x = noise(rng, 2, channels, L)
        tag = f"({n_fft},{hop},{n_mels}) L {L} x{channels}"
        got, intact = run_kernel(torch, ctx, x, sp[None])
        assert intact, tag
        M, dM = check_power(got, x, sp[None], tag, twin=True)
        for log in ("ln", "log10"):
            got, intact = run_kernel(torch, ctx, x, sp[log])
            assert intact, (tag, log)
            check_log_any(got, M, dM, sp[log], tag)


@pytest.mark.parametrize("n_fft,hop,n_mels", [(400, 160, 80), (63, 7, 12)])
def test_many_tiles_every_frame(gpu, n_fft, hop, n_mels):
    """Five tiles (four full ones and seven frames) of three rows of two channels: 30 workgroups, and five is odd, so every
    rotation of the waves (blockIdx.x & 3) meets every tile index; every frame of every tile is held against the
    specification and the twin"""
    torch, pkg, ctx = gpu
    tile = kernel_tile(n_fft, hop)
    L = (4 * tile + 6) * hop + 3
    sp = specs(n_fft, hop, n_mels)
    assert sp[None].frames(L) == 4 * tile + 7
    assert len({(b & 3, b % 5) for b in range(3 * 2 * 5)}) == 4 * 5           # blockIdx.x = plane * tiles + tile index
    x = noise(np.random.default_rng(hop), 3, 2, L)
    tag = f"({n_fft},{hop},{n_mels}) 5 tiles x 3 x 2"
    got, intact = run_kernel(torch, ctx, x, sp[None])
    assert intact
    M, dM = check_power(got, x, sp[None], tag, twin=True)
    got, intact = run_kernel(torch, ctx, x, sp["ln"])
    assert intact
    check_log_any(got, M, dM, sp["ln"], tag)


@pytest.mark.parametrize("n_fft,hop,n_mels", [(400, 160, 80), (25, 10, 8), (16, 1, 4), (2048, 562, 64)])
def test_a_frame_does_not_depend_on_where_it_sits(gpu, n_fft, hop, n_mels):
    """log_mel(x[k hop:])[..., t] == log_mel(x)[..., t + k] bit for bit, k a tile and five frames, for every t whose window is
    inside both signals (no reflection): another lane, another tile and another wave rotation do the same arithmetic"""
    torch, pkg, ctx = gpu
    tile = kernel_tile(n_fft, hop)
    k = tile + 5
    tail = max(3 * n_fft, 40 * hop)
    L = k * hop + tail
    x = noise(np.random.default_rng(n_fft + hop), 2, 1, L)
    t = np.arange(1 + tail // hop)
    ok = (t * hop >= n_fft // 2) & (t * hop - n_fft // 2 + n_fft <= tail)
    assert ok.sum() >= 8 and k % tile == 5
    for log in (None, "ln"):
        sp = specs(n_fft, hop, n_mels)[log]
        whole, intact = run_kernel(torch, ctx, x, sp)
        assert intact
        part, intact = run_kernel(torch, ctx, np.ascontiguousarray(x[:, :, k * hop:]), sp)
        assert intact and part.shape[-1] == len(t)
        assert np.isfinite(part).all() and np.isfinite(whole).all()
        assert np.array_equal(bits(part[..., ok]), bits(whole[..., t[ok] + k])), (n_fft, hop, log)
        assert not np.array_equal(bits(part[..., 0]), bits(whole[..., k]))          # (the first frame reflects: the test can fail)


@pytest.mark.parametrize("n_fft,hop,n_mels,L", [(2048, 560, 256, 20000), (18, 3, 5, 60)])
def test_a_batch_is_its_planes_run_alone(gpu, n_fft, hop, n_mels, L):
    torch, pkg, ctx = gpu
    x = noise(np.random.default_rng(L), 3, 2, L)
    for log in (None, "ln"):
        sp = specs(n_fft, hop, n_mels)[log]
        whole, intact = run_kernel(torch, ctx, x, sp)
        assert intact and np.isfinite(whole).all()
        for r in range(3):
            for c in range(2):
                one, intact = run_kernel(torch, ctx, x[r:r + 1, c:c + 1], sp)
                assert intact and np.array_equal(bits(one[0, 0]), bits(whole[r, c])), (r, c, log)


def test_log_and_floor_on_any_input(gpu):
    """The log where its interval is not narrow everywhere: filter rows of zeros (M = 0: the floor's log), a quiet signal
    around a floor that clamps part of a row, a floor above everything, and a caller's filterbank with negative weights
    (M < 0 gives the floor's log too)"""
    torch, pkg, ctx = gpu
    from alac.net_amd.features import LogMel

    rng = np.random.default_rng(17)
    # rows of zeros
    sp = specs(400, 160, 256)
    x = noise(rng, 2, 1, 3000)
    got, intact = run_kernel(torch, ctx, x, sp[None])
    M, dM = check_power(got, x, sp[None], "(400,160,256)", twin=True)
    assert intact and (M == 0).any()
    for log in ("ln", "log10"):
        got, intact = run_kernel(torch, ctx, x, sp[log])
        assert intact
        pinned = check_log_any(got, M, dM, sp[log], "(400,160,256)")
        assert np.array_equal(pinned, M == 0)
    # amplitude 1e-3 under filters with their peaks at 1 (norm=None): the mel power is 1e-6 of full scale's, 3e-6 to 6e-4, and
    # the floor of 1e-4 cuts through most rows; with the Slaney norm all of it would lie below
    x = (noise(rng, 2, 1, 5000) * np.float32(1e-3)).astype(np.float32)
    quiet = specs(400, 160, 80, norm=None)[None]
    got, intact = run_kernel(torch, ctx, x, quiet)
    M, dM = check_power(got, x, quiet, "1e-3")
    assert intact
    for floor, some_free in ((1e-4, True), (1.0, False)):
        for log in ("ln", "log10"):
            sp = LogMel(16000, 400, 160, 80, norm=None, log=log, floor=floor)
            got, intact = run_kernel(torch, ctx, x, sp)
            assert intact
            pinned = check_log_any(got, M, dM, sp, "1e-3")
            # clamped and free elements share rows (mel rows, over the frames) -- or all are clamped
            mixed = (pinned.any(axis=-1) & ~pinned.all(axis=-1)).sum()
            assert (mixed >= 80) if some_free else pinned.all(), (floor, int(mixed))
    # negative weights
    fb = rng.uniform(0.0, 1.0, (12, 201)).astype(np.float32)
    fb[1] = -fb[1]                                               # M < 0 everywhere
    fb[2, ::2] = -fb[2, ::2]                                     # either sign, small against dM's |fb|
    fb[4, :100] = -fb[4, :100] * np.float32(0.01)                # positive, a little taken off
    x = noise(rng, 2, 1, 3000)
    got, intact = run_kernel(torch, ctx, x, LogMel(16000, 400, 160, filterbank=fb, log=None))
    M, dM = check_power(got, x, LogMel(16000, 400, 160, filterbank=fb, log=None), "negative weights")
    assert intact and (M[:, :, 1] < 0).all() and (M[:, :, 2] < 0).any() and (M[:, :, 2] > 0).any() and (M[:, :, 4] > 0).all()
    sp = LogMel(16000, 400, 160, filterbank=fb, log="ln", floor=1e-3)
    got, intact = run_kernel(torch, ctx, x, sp)
    assert intact
    pinned = check_log_any(got, M, dM, sp, "negative weights")
    assert pinned[:, :, 1].all() and (pinned == (M + dM < float(np.float32(1e-3)))).all()


def test_what_is_not_finite_stays_in_its_frames_and_is_never_hidden(gpu):
    """A NaN in one row and an infinity in another, in the middle tile of three, a clean row between and behind them: the
    frames with a tap on the sample are what the specification says (features.py: NaN, with a log too -- never log(floor)),
    every other frame and every other plane is bit for bit the clean signal's"""
    torch, pkg, ctx = gpu
    from alac.net_amd.features import logmel_host

    n_fft, hop, n_mels = 400, 160, 80
    tile = kernel_tile(n_fft, hop)
    L = (2 * tile + 6) * hop
    i = (tile + 9) * hop + 30
    clean = noise(np.random.default_rng(23), 4, 1, L)
    x = clean.copy()
    x[0, 0, i] = np.nan
    x[2, 0, i] = np.inf
    t = np.arange(1 + L // hop)
    hit = (t * hop - n_fft // 2 <= i) & (i < t * hop - n_fft // 2 + n_fft)
    assert len(t) == 2 * tile + 7 and hit.sum() == 3 and (t[hit] // tile == 1).all()
    for log in (None, "ln", "log10"):
        sp = specs(n_fft, hop, n_mels)[log]
        want, intact = run_kernel(torch, ctx, clean, sp)
        assert intact and np.isfinite(want).all()
        got, intact = run_kernel(torch, ctx, x, sp)
        assert intact
        with np.errstate(invalid="ignore"):
            spec = logmel_host(x, sp)
        assert np.isnan(spec[0, 0][:, hit]).all() and np.isnan(spec[2, 0][:, hit]).all()
        for row in (0, 2):
            assert np.isnan(got[row, 0][:, hit]).all(), (log, row)
            assert np.array_equal(bits(got[row, 0][:, ~hit]), bits(want[row, 0][:, ~hit])), (log, row)
        assert np.array_equal(bits(got[1]), bits(want[1])) and np.array_equal(bits(got[3]), bits(want[3])), log


@pytest.mark.parametrize("n,hop", [(64, 16), (400, 100), (50, 5), (16, 1)])
def test_the_fbank_entry_is_the_logmel_entry_on_the_same_tables(gpu, n, hop):
    """alacgpu_fbank_device with win_length = n_fft = n, snip_edges, use_power, no mean, no pre-emphasis and scale 1 on LogMel's
    three tables against alacgpu_logmel_device without a log: fbank's frame t begins at sample t hop, log-mel's frame
    t + n / (2 hop) does too and reflects nothing, so they are bit for bit equal -- 1 * x and x - 0 are exact, the B operand is
    the same single product, the chains run in the same order, and a frame's arithmetic does not depend on its place in a tile
    (the two calls put it at different ones).  (64, 16): an even hop, a skewed span, three tiles; (400, 100): the speech
    window, seven bin blocks in one round; (50, 5): an odd hop without skew, and K = 50 leaves one whole k-step to the remainder
    loop; (16, 1): the hop-1 start of (q, r)."""
    torch, pkg, ctx = gpu
    from alac.net_amd.fbank import FLAG_SNIP_EDGES, FLAG_USE_POWER
    from alac.net_amd.features import LogMel

    dev = torch.device("cuda", 0)
    sp = LogMel(16000, n, hop, n_mels=8, log=None)
    shift, frames, slack = n // (2 * hop), 71, 37
    L = n + (frames - 1) * hop
    assert shift * 2 * hop == n and sp.frames(L) >= frames + shift
    x = noise(np.random.default_rng(n + hop), 1, 1, L)
    src = np.full((1, 1, L + slack), np.nan, dtype=np.float32)
    src[:, :, :L] = x
    d_src = torch.from_numpy(src).to(dev)
    window, basis, fb = sp.device_tables(dev)
    stream = torch.cuda.current_stream().cuda_stream

    def guarded(count):
        raw = torch.full(((count + 2 * GUARD) * 4,), 0x5A, dtype=torch.uint8, device=dev).view(torch.float32)
        raw[GUARD:GUARD + count].fill_(float("nan"))
        return raw

    def result(raw, count, T):
        torch.cuda.synchronize()
        host = raw.cpu().numpy()
        edge = np.full(GUARD * 4, 0x5A, dtype=np.uint8)
        assert np.array_equal(host[:GUARD].view(np.uint8), edge) and np.array_equal(host[GUARD + count:].view(np.uint8), edge)
        return host[GUARD:GUARD + count].reshape(sp.n_mels, T)

    Tl = sp.frames(L)
    raw = guarded(sp.n_mels * Tl)
    ctx.logmel_device(d_src, 1, 1, L + slack, L, n, hop, sp.n_mels, window, basis, fb, 0, sp.floor, raw[GUARD:GUARD + sp.n_mels * Tl], Tl,
                      stream=stream)
    logmel = result(raw, sp.n_mels * Tl, Tl)
    raw = guarded(sp.n_mels * frames)
    ctx.fbank_device(d_src, 1, 1, L + slack, L, n, n, hop, sp.n_mels, window, basis, fb, FLAG_SNIP_EDGES | FLAG_USE_POWER, 0.0, 1.0,
                     raw[GUARD:GUARD + sp.n_mels * frames], frames, stream=stream)
    fbank = result(raw, sp.n_mels * frames, frames)
    assert np.isfinite(fbank).all() and (fbank > 0).any()
    assert np.array_equal(fbank.view(np.uint32), np.ascontiguousarray(logmel[:, shift:shift + frames]).view(np.uint32)), (n, hop)
