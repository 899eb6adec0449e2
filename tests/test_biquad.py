"""alacgpu_biquad_device on the GPU against alac.net_amd/biquad.py: the kernel is its twin bit for bit and within 2^-24 |s| + D of
the sequential specification s, over the lengths around a chunk and a tile, one and two channels, 1, 3 and 8 sections, rows of
full, partial and no length, contiguous rows and slices with aligned and odd strides; the two filters float32 cannot do; in
place, twice, identity rows, sentinels, NaNs, the clamp, the gain and the coefficient forms; the C ABI's refusals one by one."""
import ctypes
import sys

import numpy as np
import pytest

from test_biquad_spec import HARD, noise, stable_sections

U32 = 2.0 ** -24
SENT = 1234.5


@pytest.fixture(scope="module")
def env():
    import torch

    import alac.net_amd as pkg

    return torch, pkg, sys.modules["alac.net_amd.biquad"]


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def sections(S):
    """The same sections for every case, so that the specification's tables are made once"""
    return stable_sections(np.random.default_rng(11), (3, 8))[:, :S].copy()


def layouts(torch, x):
    """x [B, C, T] on the device as a contiguous tensor and as slices of wider ones with an aligned and an odd stride"""
    B, C, T = x.shape
    yield "contiguous", torch.from_numpy(x).cuda()
    for name, wide in (("aligned", (T + 7) // 4 * 4), ("odd", T + 1 + T % 2)):
        w = torch.full((B, C, wide), SENT, device="cuda")
        w[..., :T] = torch.from_numpy(x).cuda()
        yield name, w[..., :T]


@pytest.mark.gpu
def test_the_constants_are_the_headers(env):
    from test_features import header_constant

    torch, pkg, bq = env
    for c in ("CHUNK", "THREADS", "LEVELS", "MAX_SECTIONS", "TILE"):
        assert getattr(bq, c) == header_constant("ALAC_BIQUAD_" + c, "alac_biquad.h"), c
    for n in ("Effects", "RandomBiquad", "biquad", "biquad_host", "biquad_host_twin", "lowpass", "highshelf"):
        assert hasattr(pkg, n)
    assert len(pkg.SYMBOLS["alacgpu_biquad_device"][1]) == 13 and hasattr(pkg.AlacGpuContext, "biquad_device")


def lengths_grid():
    from alac.net_amd.biquad import CHUNK, TILE       # (the module: the package's attribute of that name is the function)

    return [1, 2, 3, CHUNK - 1, CHUNK, CHUNK + 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 5]


@pytest.mark.gpu
@pytest.mark.parametrize("T", lengths_grid())
def test_the_kernel_is_its_twin_and_within_the_bound(env, T):
    torch, pkg, bq = env
    x2 = noise((3, 2, T), T)
    lengths = np.array([T, T // 2 + 1, 0])
    gain = np.array([0.5, 2.0, 1.5])
    for S in (1, 3, 8):
        q = sections(S)
        s2, D2 = pkg.biquad_host(x2, q, lengths, gain, bound=True)       # (channels are independent: one channel is its slice)
        twin2 = pkg.biquad_host_twin(x2, q, lengths, gain)
        for C in (1, 2):
            x, s, D, twin = x2[:, :C], s2[:, :C], D2[:, :C], twin2[:, :C]
            for name, d in layouts(torch, np.ascontiguousarray(x)):
                got = pkg.biquad(d, q, lengths, gain).cpu().numpy()
                assert np.array_equal(bits(got), bits(twin)), (T, S, C, name, np.abs(got - twin).max())
                err = np.abs(got.astype(np.float64) - s)
                assert np.all(err <= U32 * np.abs(s) + D), (T, S, C, name, float(err.max()), float(D.max()))
                if name != "contiguous":
                    assert bool((d._base[..., T:] == SENT).all()), (T, S, C, name)


@pytest.mark.gpu
def test_the_two_hard_filters(env):
    torch, pkg, bq = env
    x = noise((2, 1, 32000), 0)
    q = np.stack([pkg.__dict__[kind](48000.0, f, qq)[None] for kind, f, qq in HARD])
    s, D = pkg.biquad_host(x, q, bound=True)
    got = pkg.biquad(torch.from_numpy(x).cuda(), q).cpu().numpy()
    err = np.abs(got.astype(np.float64) - s)
    print("kernel against the specification:", err.max(axis=(1, 2)), "of peaks", np.abs(s).max(axis=(1, 2)), "D:", D.max(axis=(1, 2)),
          "results that are not the specification's rounded:", (got != s.astype(np.float32)).sum(axis=(1, 2)))
    assert np.all(err <= U32 * np.abs(s) + D)
    # (D is above the peak here: the float32 rounding of the row's peak is what bites, as in tests/test_biquad_spec.py)
    peak = np.abs(s).max(axis=(1, 2), keepdims=True)
    assert np.all(err <= U32 * np.abs(s) + U32 * peak), (err.max(axis=(1, 2)), U32 * peak.ravel())
    assert np.array_equal(bits(got), bits(pkg.biquad_host_twin(x, q)))


@pytest.mark.gpu
def test_in_place_twice_identity_and_sentinels(env):
    torch, pkg, bq = env
    T = bq.TILE + 37
    x = noise((4, 2, T), 9)
    q = sections(3)
    q = np.concatenate([q, np.tile(np.array(bq.IDENTITY), (1, 3, 1))])        # row 3: the identity
    lengths = np.array([T, 100, -1, T])
    d = torch.from_numpy(x).cuda()
    want = pkg.biquad(d, q, lengths)
    assert np.array_equal(bits(want.cpu().numpy()), bits(pkg.biquad_host_twin(x, q, lengths)))
    assert torch.equal(pkg.biquad(d, q, lengths).view(torch.int32), want.view(torch.int32))          # twice
    # an identity row and the frames at or behind the lengths of a sentinel-filled out are not written
    out = torch.full_like(d, SENT)
    assert pkg.biquad(d, q, lengths, out=out) is out
    assert bool((out[3] == SENT).all()) and bool((out[2] == SENT).all()) and bool((out[1, :, 100:] == SENT).all())
    assert torch.equal(out[0], want[0]) and torch.equal(out[1, :, :100], want[1, :, :100])
    # in place
    e = d.clone()
    assert pkg.biquad(e, q, lengths, out=e) is e and torch.equal(e.view(torch.int32), want.view(torch.int32))
    # gain=None is a gain of 1, the [S, 5] form the expanded one, device coefficients as they are
    one = pkg.biquad(d, q[0])
    assert torch.equal(one, pkg.biquad(d, np.tile(q[0], (4, 1, 1)), gain=np.ones(4)))
    assert torch.equal(one, pkg.biquad(d, torch.from_numpy(q[0]).cuda(), gain=torch.ones(4, device="cuda")))
    # the clamp
    loud = pkg.biquad(d, q, lengths, gain=[30.0, 30.0, 1.0, 30.0], clamp=True)
    assert float(loud.abs().max()) == 1.0
    assert np.array_equal(bits(loud.cpu().numpy()), bits(pkg.biquad_host_twin(x, q, lengths, [30.0, 30.0, 1.0, 30.0], clamp=True)))


@pytest.mark.gpu
def test_a_nan_stays_where_it_is(env):
    torch, pkg, bq = env
    T, n0 = bq.TILE + 300, bq.TILE + 70
    x = noise((2, 2, T), 4)
    q = sections(3)[:2]
    lengths = np.array([T, bq.TILE + 200])
    clean = pkg.biquad(torch.from_numpy(x).cuda(), q, lengths, clamp=True).cpu().numpy()
    bad = x.copy()
    bad[0, 1, n0] = np.nan                  # below v of row 0, channel 1
    bad[1, 0, bq.TILE + 200] = np.nan       # at v of row 1: never read
    got = pkg.biquad(torch.from_numpy(bad).cuda(), q, lengths, clamp=True).cpu().numpy()
    assert np.isnan(got[0, 1, n0]) and np.isnan(got[0, 1, n0:]).all()          # (a recursive filter keeps it, and so does the clamp)
    keep = np.ones(x.shape, dtype=bool)
    keep[0, 1, n0:] = False
    keep[1, 0, bq.TILE + 200] = False       # (untouched: the output holds the input's NaN there)
    assert np.array_equal(bits(got)[keep], bits(clean)[keep])
    twin = pkg.biquad_host_twin(bad, q, lengths, clamp=True)          # (which NaN it is -- its sign and payload -- is not specified)
    assert np.array_equal(np.isnan(got), np.isnan(twin)) and np.array_equal(bits(got)[~np.isnan(got)], bits(twin)[~np.isnan(twin)])


@pytest.mark.gpu
def test_what_biquad_refuses(env):
    torch, pkg, bq = env
    d = torch.zeros(2, 2, 8, device="cuda")
    q = np.tile(np.array(bq.IDENTITY), (2, 1, 1))
    for args in ((d.cpu(), q), (d.double(), q), (d[0], q), (d[..., ::2], q), (d, q[:, :, :4]), (d, np.zeros((2, 9, 5))), (d, q[:1]),
                 (d, "flat"), (d, q, [1, 2, 3]), (d, q, [1.0, 2.0]), (d, q, None, [1.0]), (d, q, None, None, 1)):
        with pytest.raises(ValueError):
            pkg.biquad(*args)
    for out in (d[..., :-1], d.double(), d.cpu(), torch.empty(2, 2, 9, device="cuda")[..., :8]):
        with pytest.raises(ValueError):
            pkg.biquad(d, q, out=out)
    assert pkg.biquad(torch.zeros(0, 2, 8, device="cuda"), np.zeros((0, 1, 5))).shape == (0, 2, 8)


@pytest.mark.gpu
def test_the_c_abi_refuses_item_by_item(env):
    torch, pkg, bq = env
    rows, C, stride, T, S = 3, 2, 16, 10, 2
    src = torch.zeros(rows * C * stride + 8, device="cuda")
    out = torch.full((rows * C * stride + 8,), 7.0, device="cuda")
    q = torch.tensor(bq.IDENTITY, dtype=torch.float64, device="cuda").repeat(rows + 1, S, 1) * 0.5
    valid = torch.full((rows + 1,), T, dtype=torch.int64, device="cuda")
    gain = torch.ones(rows + 1, dtype=torch.float64, device="cuda")
    base = dict(d_src=src.data_ptr(), d_out=out.data_ptr(), rows=rows, channels=C, stride=stride, frames=T, d_valid=valid.data_ptr(),
                d_coeffs=q.data_ptr(), sections=S, d_gain=gain.data_ptr(), clamp=0, stream=None)
    extent = 4 * ((rows * C - 1) * stride + T)
    cases = [dict(d_src=None), dict(d_out=None), dict(d_coeffs=None), dict(d_src=base["d_src"] + 2), dict(d_out=base["d_out"] + 2),
             dict(d_valid=base["d_valid"] + 4), dict(d_coeffs=base["d_coeffs"] + 4), dict(d_gain=base["d_gain"] + 4),
             dict(channels=0), dict(sections=0), dict(sections=9), dict(frames=0), dict(frames=stride + 1), dict(stride=T - 1),
             dict(d_out=base["d_src"] + 4), dict(d_out=base["d_src"] + extent - 4), dict(d_coeffs=base["d_out"]),
             dict(d_coeffs=base["d_out"] + extent - 8), dict(d_gain=base["d_out"] + 8), dict(stride=1 << 58),
             dict(d_out=base["d_src"], d_coeffs=base["d_src"] + (1 << 44), d_gain=None, rows=1 << 31, channels=1, stride=1, frames=1)]
    fn = pkg.lib().alacgpu_biquad_device
    with pkg.AlacGpuContext([(512, 16, 40, 10, 14, 2)]) as ctx:
        for change in cases:
            assert fn(ctx._ctx, *dict(base, **change).values()) == -1, change
        torch.cuda.synchronize()
        assert bool((out == 7.0).all()) and bool((src == 0).all())
        # ... and the same arguments unchanged are a call, as is one of no rows, of no lengths and of no gain
        assert fn(ctx._ctx, *dict(base, rows=0).values()) == 0
        assert fn(ctx._ctx, *dict(base, d_valid=None, d_gain=None).values()) == 0
        assert fn(ctx._ctx, *base.values()) == 0
        torch.cuda.synchronize()
    got = out[:rows * C * stride].view(rows, C, stride).cpu()
    assert bool((got[:, :, :T] == 0).all()) and bool((got[:, :, T:] == 7.0).all())


def test_a_null_ctx_is_refused_without_a_device():
    import alac.net_amd as pkg

    args = dict(d_src=0x10000, d_out=0x20000, rows=3, channels=2, stride=16, frames=10, d_valid=0x40000, d_coeffs=0x50000, sections=2,
                d_gain=0x60000, clamp=0, stream=None)
    fn = pkg.lib().alacgpu_biquad_device
    assert fn(None, *args.values()) == -1 and fn(None, *dict(args, rows=0).values()) == -1
    page = ctypes.create_string_buffer(4096)
    assert fn(ctypes.addressof(page), *dict(args, rows=0).values()) == 0              # no rows: nothing of the ctx is needed
    assert fn(ctypes.addressof(page), *dict(args, rows=0, sections=9).values()) == -1
