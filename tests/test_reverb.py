"""alacgpu_reverb_device on the GPU against its specification in numpy (alac.net_amd/reverb.py), then `reverb`.

Three criteria per call, y and dY from reverb_host(..., bound=True) and the twin t = reverb_host_f32:
  |got - y| <= dY for every element below v;
  r_gpu <= 4 r_twin with r = max |. - y| / dY over the elements with a positive dY -- the factor of tests/test_features.py
  and tests/test_normalize.py;
  got is x bit for bit for every element at or behind v and for every row the specification leaves alone.

Every call reads a source and responses whose planes carry NaN behind `frames` and `rir_frames` (a slack of 5 floats, which
puts most planes off 16 bytes, and the slack that puts every plane at a multiple of 16 bytes) and writes into an output
prefilled with NaN between guards of 0x5A bytes: the guards, what lies behind `frames` in the output, the responses and -- out
of place -- the source are intact after every call.  Shapes are chosen by code path, around the hop H = N / 2 of
csrc/alac_reverb.h: one block, the last frame of a block, the first of the next, several blocks and partitions."""
import numpy as np
import pytest

from test_features import header_constant
from test_mix import GUARD, NAN, SLACK, padded, wide
from test_normalize_spec import noise, same_bits

pytestmark = pytest.mark.gpu

N = header_constant("ALAC_REVERB_N", "alac_reverb.h")
H = N // 2


@pytest.fixture(scope="module")
def gpu():
    import torch

    import alac.net_amd as pkg

    with pkg.AlacGpuContext([(4096, 16, 40, 10, 14, 2)], device=0) as ctx:
        yield torch, ctx


def run(gpu, x, h, valid=None, hvalid=None, slack=SLACK, hslack=SLACK, in_place=False):
    """One ctx.reverb_device call over x [rows, C, frames] and h [rows, Ch, rir_frames] (numpy float32): both with NaN behind
    every plane, the output of the source's layout prefilled with NaN between two guards (in_place: the source lives there).
    Returns out [rows, C, frames] as numpy after checking the guards, what lies behind the planes, the responses and the
    source."""
    torch, ctx = gpu
    dev = torch.device("cuda", 0)
    rows, C, T = x.shape
    K = h.shape[2]
    S, Sh = T + slack, K + hslack
    total = rows * C * S
    raw = torch.full(((total + 2 * GUARD) * 4,), 0x5A, dtype=torch.uint8, device=dev).view(torch.float32)
    out = raw[GUARD:GUARD + total]
    d_src = torch.from_numpy(padded(x, slack)).to(dev)
    d_rir = torch.from_numpy(padded(h, hslack)).to(dev)
    if in_place:
        out.copy_(d_src.flatten())
        d_src = out
    else:
        out.fill_(NAN)
    as_dev = lambda v: None if v is None else torch.tensor(list(v), dtype=torch.int64, device=dev)
    ctx.reverb_device(d_src, out, d_rir, rows, C, h.shape[1], S, Sh, T, K, as_dev(valid), as_dev(hvalid),
                      stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert bool((torch.cat([raw[:GUARD], raw[GUARD + total:]]).view(torch.uint8) == 0x5A).all()), "a guard was written"
    got = out.cpu().numpy().reshape(rows, C, S)
    assert np.isnan(got[:, :, T:]).all(), "an element behind frames was written"
    back = d_rir.cpu().numpy()
    assert np.array_equal(back[:, :, :K], h, equal_nan=True) and np.isnan(back[:, :, K:]).all(), "the responses were written"
    if not in_place:
        back = d_src.cpu().numpy()
        assert np.array_equal(back[:, :, :T], x, equal_nan=True) and np.isnan(back[:, :, T:]).all(), "the source was written"
    return got[:, :, :T].copy()


REFS = {}


def reference(key, x, h, valid, hvalid):
    """(y, dY, twin) of an input, computed once per key and shared"""
    from alac.net_amd.reverb import reverb_host, reverb_host_f32

    if key not in REFS:
        y, dY = reverb_host(x, h, valid, hvalid, bound=True)
        t = reverb_host_f32(x, h, valid, hvalid)
        for a in (y, dY, t):
            a.setflags(write=False)
        REFS[key] = (y, dY, t)
    return REFS[key]


def stays(x, h, valid, hvalid):
    """The elements the specification leaves as they are: at or behind v, and the rows it leaves alone"""
    rows, C, T = x.shape
    K = h.shape[2]
    mask = np.zeros(x.shape, dtype=bool)
    for b in range(rows):
        v = T if valid is None else min(max(valid[b], 0), T)
        vh = K if hvalid is None else min(max(hvalid[b], 0), K)
        mask[b, :, v:] = True
        if v == 0 or vh == 0 or not np.any(h[b, :, :vh]):
            mask[b] = True
    return mask


def check(got, ref, x, h, valid, hvalid, tag):
    y, dY, t = ref
    keep = stays(x, h, valid, hvalid)
    assert np.array_equal(got[keep].view(np.int32), x[keep].view(np.int32)), (tag, "an element that stays is not x bit for bit")
    assert not dY[keep].any() and (dY[~keep] > 0).all(), tag
    live = ~keep & np.isfinite(y)
    err = np.abs(got.astype(np.float64) - y)
    r_gpu = float(np.max(err[live] / dY[live])) if live.any() else 0.0
    r_twin = float(np.max(np.abs(t.astype(np.float64) - y)[live] / dY[live])) if live.any() else 0.0
    print(f"{tag}: max err {float(err[live].max()) if live.any() else 0.0:.3e}, r_gpu {r_gpu:.3e}, r_twin {r_twin:.3e}, equal bits {same_bits(got, t)}")
    assert np.isfinite(got[live]).all() and (err[live] <= dY[live]).all(), (tag, r_gpu)
    assert r_gpu <= 4 * r_twin, (tag, r_gpu, r_twin)


def responses(rows, Ch, K, seed, where):
    """Decaying noise with the direct path, a tap of 2, at where[b] of 'first', 'middle', 'last' of the valid frames"""
    rng = np.random.default_rng(seed)
    return (0.3 * rng.standard_normal((rows, Ch, K)) * np.exp(-np.arange(K) / max(K / 5.0, 1.0))).astype(np.float32)


def place_direct(h, hvalid, where):
    for b, w in enumerate(where):
        vh = min(max(hvalid[b], 0), h.shape[2])
        if vh:
            h[b, 0, {"first": 0, "middle": vh // 2, "last": vh - 1}[w]] = 2.0
    return h


def case(T, K, C, Ch, rows, turn):
    """(x, h, valid, hvalid) with another selection of v, vh and d in every row and every turn"""
    vpool = [T, T - 1, 1, T + 3, 0, T, -2, max(T // 2, 1)]
    hpool = [K, K, 1, K, 0, max(K - 1, 1)]
    wpool = ["middle", "first", "last"]
    valid = [vpool[(turn + 3 * b) % len(vpool)] for b in range(rows)]
    hvalid = [hpool[(turn + 2 * b) % len(hpool)] for b in range(rows)]
    where = [wpool[(turn + b) % 3] for b in range(rows)]
    x = noise((rows, C, T), 100 + T + K + C)
    h = place_direct(responses(rows, Ch, K, 200 + T + K + Ch, where), hvalid, where)
    return x, h, valid, hvalid


FRAMES = [1, H - 1, H, H + 1, 2 * H + 5]
RIR_FRAMES = [1, 2, H, H + 1, 2 * H + 3]


@pytest.mark.parametrize("T", FRAMES)
@pytest.mark.parametrize("K", RIR_FRAMES)
def test_grid_of_frames_responses_channels_and_layouts(gpu, T, K):
    """Frames and response frames around the hop; three rows (one row for one channel pair) with their own v, vh and d; C in
    1, 2 and Ch in 1, C; planes off and at multiples of 16 bytes; every call out of place and in place"""
    turn = FRAMES.index(T) + 5 * RIR_FRAMES.index(K)
    for n, (C, Ch) in enumerate(((1, 1), (2, 1), (2, 2))):
        rows = 1 if (turn + n) % 3 == 0 else 3
        x, h, valid, hvalid = case(T, K, C, Ch, rows, turn + n)
        ref = reference((T, K, C, Ch, rows, turn + n), x, h, valid, hvalid)
        for slack, hslack in ((SLACK, SLACK), (wide(T), wide(K))):
            for in_place in (False, True):
                tag = f"T {T} K {K} C {C} Ch {Ch} valid {valid} rir valid {hvalid} slack {slack}/{hslack} in place {in_place}"
                check(run(gpu, x, h, valid, hvalid, slack, hslack, in_place), ref, x, h, valid, hvalid, tag)
    x, h, _, _ = case(T, K, 2, 1, 2, turn)
    place_direct(h, [K, K], ["middle", "last"])
    ref = reference((T, K, "whole"), x, h, None, None)
    check(run(gpu, x, h), ref, x, h, None, None, f"T {T} K {K} whole")
    check(run(gpu, x, h, slack=wide(T), hslack=SLACK, in_place=True), ref, x, h, None, None, f"T {T} K {K} whole, in place")


def kinds(T, K, C, Ch, seed):
    names = ["full", "partial", "v 0", "v -1", "vh 0", "vh -1", "silent", "plain a", "plain b", "vh 1", "beyond"]
    at = {k: i for i, k in enumerate(names)}
    B = len(names)
    x = noise((B, C, T), seed)
    valid, hvalid = [T] * B, [K] * B
    valid[at["partial"]] = T - T // 3
    valid[at["v 0"]], valid[at["v -1"]], hvalid[at["vh 0"]], hvalid[at["vh -1"]] = 0, -1, 0, -1
    hvalid[at["vh 1"]] = 1
    valid[at["beyond"]], hvalid[at["beyond"]] = T + 9, K + 9
    valid[at["plain b"]], hvalid[at["plain b"]] = T - 10, K - 3
    where = [("middle", "first", "last")[b % 3] for b in range(B)]
    h = place_direct(responses(B, Ch, K, seed + 1, where), hvalid, where)
    h[at["silent"]] = 0.0
    return x, h, valid, hvalid, at


@pytest.mark.parametrize("T,K,C,Ch", [(2 * H + 77, H + 300, 2, 1), (H + 1000, 700, 1, 1), (3001, 2 * H + 1, 2, 2)])
def test_rows_of_every_kind_in_one_call(gpu, T, K, C, Ch):
    x, h, valid, hvalid, at = kinds(T, K, C, Ch, 77 + T)
    ref = reference((T, K, C, Ch, "kinds"), x, h, valid, hvalid)
    outs = []
    for slack, hslack, in_place in ((SLACK, SLACK, False), (wide(T), wide(K), False), (SLACK, wide(K), True), (wide(T), SLACK, True)):
        got = run(gpu, x, h, valid, hvalid, slack, hslack, in_place)
        check(got, ref, x, h, valid, hvalid, f"T {T} K {K} C {C} Ch {Ch} kinds, slack {slack}/{hslack}, in place {in_place}")
        outs.append(got)
    for got in outs[1:]:                                   # a function of the inputs alone: every layout, the same bits
        assert same_bits(got, outs[0])
    got = outs[0]
    assert same_bits(run(gpu, x, h, valid, hvalid), got), "the same call twice"
    for k in ("v 0", "v -1", "vh 0", "vh -1", "silent"):
        assert np.array_equal(got[at[k]].view(np.int32), x[at[k]].view(np.int32)), k
    for k in ("full", "partial", "plain a", "plain b", "vh 1", "beyond"):
        assert not np.array_equal(got[at[k]], x[at[k]]) and np.isfinite(got[at[k]]).all(), k
    for k in ("partial", "plain b", "silent"):             # every row alone is the row of the batch
        b = at[k]
        alone = run(gpu, x[b:b + 1], h[b:b + 1], valid[b:b + 1], hvalid[b:b + 1])
        assert same_bits(alone[0], got[b]), k


def test_what_is_not_finite_stays_in_its_row(gpu):
    T, K, C, Ch = 2 * H + 77, H + 300, 2, 1
    x, h, valid, hvalid, at = kinds(T, K, C, Ch, 77 + T)
    ref = run(gpu, x, h, valid, hvalid)
    a, b = at["plain a"], at["plain b"]
    others = [r for r in range(len(at)) if r not in (a, b)]
    for bad in (np.nan, np.inf):
        z, m = x.copy(), h.copy()
        z[a, C - 1, T // 3] = bad                          # inside v of one row's signal: that channel of that row
        m[b, 0, hvalid[b] - 1] = bad                       # inside vh of another row's response: e is not finite, the row stays
        for in_place in (False, True):
            got = run(gpu, z, m, valid, hvalid, in_place=in_place)
            assert same_bits(got[others], ref[others]), (bad, in_place, "another row changed")
            assert same_bits(got[b], x[b]), (bad, "a response that is not finite leaves its row alone")
            assert same_bits(got[a, 0], ref[a, 0]) and not np.isfinite(got[a, C - 1]).all(), bad
    # at or behind v and vh, and in a row that is left alone: never read
    z, m = x.copy(), h.copy()
    p = at["partial"]
    m[b, :, hvalid[b]:] = np.nan
    m[at["v 0"]] = m[at["v -1"]] = m[at["vh 0"]] = np.nan
    z[at["v 0"]] = z[at["v -1"]] = np.nan
    z[p, :, valid[p]:] = np.inf
    for in_place in (False, True):
        got = run(gpu, z, m, valid, hvalid, in_place=in_place)
        want = ref.copy()
        want[at["v 0"]] = want[at["v -1"]] = np.nan        # (x itself)
        want[p, :, valid[p]:] = np.inf
        assert same_bits(got, want), in_place


def test_the_public_call(gpu):
    import alac.net_amd as pkg
    from alac.net_amd.reverb import reverb_host, reverb_host_f32

    torch, ctx = gpu
    B, C, T, K = 4, 2, 5000, 1500
    x = noise((B, C, T), 5)
    h = place_direct(responses(B, 1, K, 6, None), [K] * B, ["middle", "first", "last", "middle"])
    d, dh = torch.from_numpy(x).cuda(), torch.from_numpy(h).cuda()
    lengths, hlen = [T, 4000, -1, 3000], [K, 0, K, 1234]
    got = pkg.reverb(d, dh, lengths, hlen)
    assert got.shape == d.shape and got.data_ptr() != d.data_ptr() and torch.equal(d.cpu(), torch.from_numpy(x))
    # ... is what the ctx call gives
    S = torch.empty_like(d)
    ctx.reverb_device(d, S, dh, B, C, 1, T, K, T, K, torch.tensor(lengths, device="cuda"), torch.tensor(hlen, device="cuda"),
                      stream=torch.cuda.current_stream().cuda_stream)
    assert torch.equal(S.view(torch.int32), got.view(torch.int32))
    y, dY = reverb_host(x, h, lengths, hlen, bound=True)
    g = got.cpu().numpy()
    assert (np.abs(g - y) <= dY).all() and np.array_equal(g[1], x[1]) and np.array_equal(g[2], x[2]) and not np.array_equal(g[0], x[0])
    t = reverb_host_f32(x, h, lengths, hlen)
    assert np.abs(g - y).max() <= 4 * np.abs(t - y).max()
    for ln, hl in ((torch.tensor(lengths, device="cuda"), torch.tensor(hlen, dtype=torch.int32)), (np.array(lengths), np.array(hlen))):
        assert torch.equal(pkg.reverb(d, dh, ln, hl).view(torch.int32), got.view(torch.int32))
    e = d.clone()
    assert pkg.reverb(e, dh, lengths, hlen, out=e) is e and torch.equal(e.view(torch.int32), got.view(torch.int32))
    # whole rows, two channels of response
    h2 = np.concatenate([h, h[:, :, ::-1]], axis=1).copy()
    whole = pkg.reverb(d, torch.from_numpy(h2).cuda()).cpu().numpy()
    y, dY = reverb_host(x, h2, bound=True)
    assert (np.abs(whole - y) <= dY).all()
    # the slice [..., :T - 1] and [..., :K - 1] of both: the last column is neither read nor written
    z, m = x.copy(), h.copy()
    z[..., -1] = m[..., -1] = np.nan
    dz, dm = torch.from_numpy(z).cuda(), torch.from_numpy(m).cuda()
    want = pkg.reverb(torch.from_numpy(np.ascontiguousarray(x[..., :-1])).cuda(), torch.from_numpy(np.ascontiguousarray(h[..., :-1])).cuda(),
                      lengths, hlen).cpu().numpy()
    assert same_bits(pkg.reverb(dz[..., :-1], dm[..., :-1], lengths, hlen).cpu().numpy(), want)
    assert pkg.reverb(dz[..., :-1], dm[..., :-1], lengths, hlen, out=dz[..., :-1]).data_ptr() == dz.data_ptr()
    back = dz.cpu().numpy()
    assert same_bits(back[..., :-1], want) and np.isnan(back[..., -1]).all()
    assert pkg.reverb(d[:0], dh[:0]).shape == (0, C, T)
    # ValueError before any device work
    for args in ((d.cpu(), dh), (d, dh.cpu()), (d.double(), dh), (d, dh.double()), (d[0], dh[0]), (d, dh[:2]), (d, dh[..., :0]),
                 (d, torch.zeros(B, 3, K, device="cuda")), (d[..., ::2], dh), (d, dh[..., ::2]), (d, dh, [1, 2]), (d, dh, [1.0] * B),
                 (d, dh, None, torch.ones(B, device="cuda")), (d, dh, None, [1] * (B + 1)), (d, d, None, None, d)):
        with pytest.raises(ValueError):
            pkg.reverb(*args)
    for out in (d[..., :-1], d.double(), d.cpu(), torch.empty(B, C, T + 1, device="cuda")[..., :T], dh.expand(B, C, K)[..., :K]):
        with pytest.raises(ValueError):
            pkg.reverb(d, dh, out=out)
    big = torch.zeros(B, 1, T, device="cuda")
    with pytest.raises(ValueError):
        pkg.reverb(d, big, out=big.expand(B, C, T))


def test_bad_arguments_are_refused_and_nothing_is_enqueued(gpu):
    import alac.net_amd as pkg

    torch, ctx = gpu
    rows, C, S, T, Sh, K = 3, 2, 16, 10, 8, 6
    src = torch.zeros(rows * C * S + 8, device="cuda")
    out = torch.full((rows * C * S + 8,), 7.0, device="cuda")
    rir = torch.ones(rows * Sh + 8, device="cuda")
    valid, hvalid = torch.full((rows + 1,), T, dtype=torch.int64, device="cuda"), torch.full((rows + 1,), K, dtype=torch.int64, device="cuda")
    base = dict(d_src=src.data_ptr(), d_out=out.data_ptr(), d_rir=rir.data_ptr(), rows=rows, channels=C, rir_channels=1, stride=S,
                rir_stride=Sh, frames=T, rir_frames=K, d_valid=valid.data_ptr(), d_rir_valid=hvalid.data_ptr(), stream=None)
    extent = 4 * ((rows * C - 1) * S + T)
    far = 1 << 44
    cases = [dict(d_src=None), dict(d_out=None), dict(d_rir=None), dict(d_src=base["d_src"] + 2), dict(d_out=base["d_out"] + 2),
             dict(d_rir=base["d_rir"] + 1), dict(d_valid=base["d_valid"] + 4), dict(d_rir_valid=base["d_rir_valid"] + 4), dict(channels=0),
             dict(rir_channels=0), dict(rir_channels=3), dict(frames=0), dict(rir_frames=0), dict(frames=S + 1), dict(rir_frames=Sh + 1),
             dict(stride=T - 1), dict(rir_stride=K - 1), dict(d_out=base["d_src"] + 4), dict(d_out=base["d_src"] + extent - 4),
             dict(d_rir=base["d_out"]), dict(d_rir=base["d_out"] + extent - 4), dict(d_out=base["d_src"], d_rir=base["d_src"] + 16),
             dict(stride=1 << 58), dict(rir_stride=1 << 58),
             dict(d_out=base["d_src"], d_rir=base["d_src"] + far, rows=1 << 30, channels=1, stride=1, rir_stride=1, frames=1, rir_frames=1),
             dict(d_out=base["d_src"], d_rir=base["d_src"] + (1 << 50), rows=1, channels=1, stride=1 << 43, rir_stride=1, frames=1 << 43, rir_frames=1)]
    fn = pkg.lib().alacgpu_reverb_device
    for change in cases:
        assert fn(ctx._ctx, *dict(base, **change).values()) == -1, change
    assert fn(None, *base.values()) == -1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((src == 0).all())
    # ... and the same arguments unchanged are a call, as is one of no rows
    assert fn(ctx._ctx, *dict(base, rows=0).values()) == 0
    assert fn(ctx._ctx, *base.values()) == 0
    torch.cuda.synchronize()
    got = out[:rows * C * S].view(rows, C, S).cpu()
    assert bool((got[:, :, :T] == 0).all()) and bool((got[:, :, T:] == 7.0).all())      # x == 0: y = 0
