"""alacgpu_resample_device on the GPU against its specification in numpy (resample.apply_table / resample_host), element by
element.  The tolerance of an output is (N + 2) * 2^-24 * sum_k |w_k x_k|, computed from the specification: the forward
error bound of a chain of N float32 fused multiply-adds (N * u * sum |w x| to first order, u = 2^-24), one u more for the
final rounding and one for the mono add in front.  It is derived, not measured, and no element is left out."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PAIRS = [(44100, 16000), (44100, 48000), (48000, 44100), (44100, 22050), (101, 97)]
GUARD = 64


def run_kernel(torch, pkg, ctx, src, origin, valid, first, out_frames, table, mono, d_table=None):
    """The call over src [rows, C, stride] (numpy float32) into an output with GUARD elements of 0x5A bytes on both sides;
    returns (out [rows, C or 1, out_frames] numpy, guards intact)"""
    dev = torch.device("cuda", 0)
    a, b, width, d0, w = table
    rows, C_, stride = src.shape
    Co = 1 if mono else C_
    n = rows * Co * out_frames
    raw = torch.full(((n + 2 * GUARD) * 4,), 0x5A, dtype=torch.uint8, device=dev).view(torch.float32)
    out = raw[GUARD:GUARD + n]
    up = lambda x, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=dt))).to(dev)
    d_d0, d_w = d_table if d_table is not None else (up(d0, np.int32), up(w, np.float32))
    ctx.resample_device(up(src, np.float32), rows, C_, stride, up(origin, np.int64), up(valid, np.int64), up(first, np.int64),
                        out_frames, a, b, width, d_d0, d_w, mono, out, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    intact = bool((torch.cat([raw[:GUARD], raw[GUARD + n:]]).view(torch.uint8) == 0x5A).all())
    return out.cpu().numpy().reshape(rows, Co, out_frames), intact


def check_rows(src, origin, valid, first, out_frames, table, mono, got, tag):
    from alac.net_amd.resample import apply_table

    N = 2 * table[2] + 1
    stride = src.shape[-1]
    for r in range(src.shape[0]):
        v = min(max(int(valid[r]), 0), stride)
        x = src[r, :, :v].astype(np.float64)
        kw = dict(mono=mono, origin=int(origin[r]), first=int(first[r]), num_frames=out_frames)
        want = apply_table(x, *table, **kw)
        tol = (N + 2) * 2.0 ** -24 * apply_table(x, *table, magnitude=True, **kw)
        err = np.abs(got[r].astype(np.float64) - want)
        print(f"{tag} row {r}: max err {err.max():.3e}, max err / tol {np.max(err / np.maximum(tol, 1e-300)):.3f}, max |y| {np.abs(want).max():.3e}")
        assert np.isfinite(got[r]).all(), (tag, r)
        assert (err <= tol).all(), (tag, r, int(np.argmax(err - tol)), float(err.max()))


def rows_for(a, b, stride, rng, channels):
    """Eight rows: a whole signal, a later first frame, an origin the taps reach in front of, no signal, one frame, a signal
    shorter than its row, frames beyond 2^32, and a valid count above the stride and below zero"""
    origin = [0, 0, 5 * a + 3, 11, 7, 0, 10 ** 12, 0, 0]
    valid = [stride, stride, stride, 0, 1, stride // 3, stride, stride + 100, -5]
    first = [0, 3 * b + 1, ((5 * a + 3) * b) // a, 0, 0, 0, (10 ** 12 * b) // a - 5, 0, 0]
    src = rng.standard_normal((len(origin), channels, stride)).astype(np.float32)
    for r, v in enumerate(valid):       # what lies behind a row's signal must not matter
        if 0 <= v < stride:
            src[r, :, v:] = np.nan if r % 2 else 1e30
        if v < 0:
            src[r] = np.nan
    return src, np.array(origin), np.array(valid), np.array(first)


@pytest.mark.parametrize("r,R", PAIRS)
def test_kernel_equals_its_specification(r, R):
    import torch

    import alac.net_amd as pkg
    from alac.net_amd.resample import resample_table

    table = resample_table(r, R)
    a, b = table[:2]
    rng = np.random.default_rng(r)
    out_frames = 2500
    stride = int(1800 * a / b)           # the signals end inside the output: zeros behind
    with pkg.AlacGpuContext([(4096, 16, 40, 10, 14, 2)]) as ctx:
        for channels, mono in ((1, False), (2, False), (2, True), (1, True)):
            src, origin, valid, first = rows_for(a, b, stride, rng, channels)
            got, intact = run_kernel(torch, pkg, ctx, src, origin, valid, first, out_frames, table, mono)
            assert intact, "a store outside d_out"
            assert got.shape[1] == (1 if mono else channels)
            check_rows(src, origin, valid, first, out_frames, table, mono, got, f"{r}->{R} C{channels} mono{int(mono)}")
            assert not got[3].any() and not got[8].any() and got[0].any() and not got[0][:, 1900:].any()
            again, _ = run_kernel(torch, pkg, ctx, src, origin, valid, first, out_frames, table, mono)
            assert np.array_equal(got.view(np.uint32), again.view(np.uint32))        # two calls, bit for bit


def test_tile_edges_and_wide_ratios():
    import torch

    import alac.net_amd as pkg
    from alac.net_amd.resample import identity_table, resample_table

    rng = np.random.default_rng(8)
    with pkg.AlacGpuContext([(4096, 16, 40, 10, 14, 2)]) as ctx:
        table = resample_table(44100, 16000)
        a, b = table[:2]
        # out_frames around the tile (1024) and its quarters, and many tiles per workgroup
        for out_frames in (1, 255, 256, 257, 1023, 1024, 1025, 2048, 2049, 40000):
            stride = int(out_frames * a / b) + 50
            src = rng.standard_normal((2, 2, stride)).astype(np.float32)
            origin, valid, first = np.array([0, a]), np.array([stride, stride - 9]), np.array([0, b - 1])
            got, intact = run_kernel(torch, pkg, ctx, src, origin, valid, first, out_frames, table, True)
            assert intact, out_frames
            check_rows(src, origin, valid, first, out_frames, table, True, got, f"out_frames {out_frames}")
        # ratios whose span of 1024 output frames does not fit: tiles of 256 (48 : 1) and of 128 in more than 64 KiB (200 : 1)
        for r, R, out_frames in ((48000, 1000, 700), (200000, 1000, 300)):
            table = resample_table(r, R)
            a, b = table[:2]
            stride = out_frames * a - 77
            src = rng.standard_normal((3, 1, stride)).astype(np.float32)
            origin, valid, first = np.array([0, 3, 0]), np.array([stride, stride, 5]), np.array([0, 1, 0])
            got, intact = run_kernel(torch, pkg, ctx, src, origin, valid, first, out_frames, table, False)
            assert intact, (r, R)
            check_rows(src, origin, valid, first, out_frames, table, False, got, f"{r}->{R}")
        # the table that copies: exact
        src = rng.standard_normal((2, 2, 3000)).astype(np.float32)
        origin, valid, first = np.array([0, 10]), np.array([3000, 2000]), np.array([0, 5])
        got, intact = run_kernel(torch, pkg, ctx, src, origin, valid, first, 3000, identity_table(), True)
        mean = (src[:, 0] + src[:, 1]) * np.float32(0.5)
        assert intact and np.array_equal(got[0, 0], mean[0])
        assert np.array_equal(got[1, 0, 5:2005], mean[1, :2000]) and not got[1, 0, :5].any() and not got[1, 0, 2005:].any()


def test_bad_arguments_are_refused_before_anything_is_enqueued():
    import torch

    import alac.net_amd as pkg

    L_ = pkg.lib()
    with pkg.AlacGpuContext([(4096, 16, 40, 10, 14, 2)]) as ctx:
        t = torch.zeros(16384, dtype=torch.int64, device="cuda")      # (room for the largest table)
        p, q = pkg._dp(t), pkg._VP(t.data_ptr() + 4)
        names = ["ctx", "src", "rows", "channels", "stride", "origin", "valid", "first", "out_frames", "a", "b", "width", "d0", "w",
                 "mono", "out", "stream"]
        good = dict(ctx=ctx._ctx, src=p, rows=1, channels=1, stride=64, origin=p, valid=p, first=p, out_frames=16, a=2, b=1, width=13,
                    d0=p, w=p, mono=0, out=p, stream=None)
        call = lambda **kw: L_.alacgpu_resample_device(*[{**good, **kw}[k] for k in names])
        assert call() == 0 and call(mono=1) == 0 and call(channels=2, mono=1) == 0       # mono of one channel is allowed
        assert call(rows=0) == 0 and call(out_frames=0) == 0
        for k in ("ctx", "src", "origin", "valid", "first", "d0", "w", "out"):
            assert call(**{k: None}) == -1, k
        for k in ("origin", "valid", "first"):
            assert call(**{k: q}) == -1, k                                                # 8-byte arrays at 4
        for k in ("src", "d0", "w", "out", "origin"):
            assert call(**{k: pkg._VP(t.data_ptr() + 2)}) == -1, k
        for kw in (dict(a=0), dict(b=0), dict(width=0), dict(channels=0), dict(channels=3), dict(b=160, width=51), dict(b=16385, width=1),
                   dict(b=1, width=8192)):
            assert call(**kw) == -1, kw
        assert call(b=1, width=8191, out_frames=2) == 0                                   # the largest table there is
        torch.cuda.synchronize()
        assert not t.any()                  # (zero weights over zeros: the calls that ran wrote zeros)


def test_resample_of_load_and_load_batch(synth):
    import torch

    import alac.net_amd as pkg
    from alac.net_amd.resample import resample_host, resample_table
    from test_load_window import make_file

    files = [make_file(synth, n, last, ss, True, seed=20 + i)[0] for i, (n, last, ss) in enumerate([(3, 100, 16), (2, 4000, 24), (1, 9, 16)])]
    pcm, lengths, rate = pkg.load_batch(files)
    assert rate == 44100
    N = 2 * resample_table(44100, 16000)[2] + 1
    for mono in (False, True):
        out, new_lengths = pkg.resample(pcm, rate, 16000, lengths=lengths, mono=mono)
        assert new_lengths.tolist() == [-(-160 * int(n) // 441) for n in lengths] and new_lengths.dtype == torch.int64
        assert out.shape == (3, 1 if mono else 2, -(-160 * pcm.shape[2] // 441)) and out.dtype == torch.float32
        for f in range(3):
            n, m = int(lengths[f]), int(new_lengths[f])
            x = pcm[f, :, :n].cpu().numpy().astype(np.float64)
            want = resample_host(x, rate, 16000, mono=mono)
            tol = (N + 2) * 2.0 ** -24 * resample_host(x, rate, 16000, mono=mono, magnitude=True)
            got = out[f].cpu().numpy().astype(np.float64)
            assert (np.abs(got[:, :m] - want) <= tol).all() and not got[:, m:].any(), (mono, f)
    one, _ = pkg.load(files[0])
    y = pkg.resample(one, 44100, 48000)
    x = one.cpu().numpy().astype(np.float64)
    N = 2 * resample_table(44100, 48000)[2] + 1
    assert y.shape == (2, -(-160 * one.shape[1] // 147))
    assert (np.abs(y.cpu().numpy() - resample_host(x, 44100, 48000)) <= (N + 2) * 2.0 ** -24 * resample_host(x, 44100, 48000, magnitude=True)).all()
    # equal rates: the input itself, nothing launched; mono alone: the mean, exactly
    same, same_lengths = pkg.resample(pcm, 44100, 44100, lengths=lengths)
    assert same is pcm and same_lengths.tolist() == lengths.tolist()
    mean, _ = pkg.resample(pcm, 44100, 44100, lengths=lengths, mono=True)
    keep = torch.arange(pcm.shape[2], device="cuda")[None, :] < lengths.to("cuda")[:, None]
    assert torch.equal(mean[:, 0], torch.where(keep, (pcm[:, 0] + pcm[:, 1]) * 0.5, 0))
    for bad in (dict(pcm=pcm.cpu()), dict(pcm=pcm.to(torch.int32)), dict(pcm=pcm[0], lengths=[5]), dict(lengths=[1, 2]), dict(new_rate=0)):
        with pytest.raises(ValueError):
            pkg.resample(**{**dict(pcm=pcm, orig_rate=44100, new_rate=16000), **bad})
