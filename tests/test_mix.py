"""alacgpu_mix_device on the GPU against its specification in numpy (alac.net_amd/mix.py), then `mix`.

Three criteria per call, y and dY from mix_host(..., bound=True) and the twin t = mix_host_f32:
  |got - y| <= dY for every element (where y is not finite, got is y);
  r_gpu <= 4 r_twin with r = max |. - y| / dY over the elements with a finite, positive dY -- the factor of
  tests/test_normalize.py and tests/test_features.py;
  got equals t bit for bit (zeros comparing equal, NaN equal to NaN).  That holds for EVERY case here, not for some: the
  order of the kernel's sums (csrc/alac_mix.h) is a function of frames and the lengths alone -- the partial a frame goes to,
  the trees and the order of the parts do not change with the width of the loads, with the strides, with channels or with
  in-place -- and every other operation is rounded exactly once.

Every call reads a source and a noise whose planes carry NaN behind `frames` (a slack of 5 floats, which puts most planes off
16 bytes: the 4-byte path; and the slack that puts every plane at a multiple of 16 bytes: the 16-byte path) and writes into
an output prefilled with NaN between guards of 0x5A bytes: the guards, what lies behind `frames` in the output, the noise
and -- out of place -- the source are intact after every call.  Shapes are chosen by code path: both sides of every threshold
of csrc/alac_mix.h."""
import numpy as np
import pytest

from test_features import header_constant
from test_normalize_spec import noise, same_bits

pytestmark = pytest.mark.gpu

GUARD = 64
SLACK = 5
NAN = float("nan")


def constant(name):
    return header_constant(name, "alac_mix.h")


@pytest.fixture(scope="module")
def gpu():
    import torch

    import alac.net_amd as pkg

    with pkg.AlacGpuContext([(4096, 16, 40, 10, 14, 2)], device=0) as ctx:
        yield torch, ctx


def wide(frames):
    """The slack of 1 .. 4 floats that makes a plane's stride a multiple of 16 bytes"""
    return (-frames) % 4 or 4


def padded(a, slack):
    rows, ch, n = a.shape
    p = np.full((rows, ch, n + slack), np.nan, dtype=np.float32)
    p[:, :, :n] = a
    return p


def run(gpu, x, n, ratio, valid=None, nvalid=None, slack=SLACK, nslack=SLACK, in_place=False):
    """One ctx.mix_device call over x [rows, C, frames] and n [rows, Cn, frames] (numpy float32): both with NaN behind every
    plane, the output of the source's layout prefilled with NaN between two guards (in_place: the source lives there).
    Returns out [rows, C, frames] as numpy after checking the guards, what lies behind the planes, the noise and the source."""
    torch, ctx = gpu
    dev = torch.device("cuda", 0)
    rows, C, T = x.shape
    S, Sn = T + slack, T + nslack
    total = rows * C * S
    raw = torch.full(((total + 2 * GUARD) * 4,), 0x5A, dtype=torch.uint8, device=dev).view(torch.float32)
    out = raw[GUARD:GUARD + total]
    src = padded(x, slack)
    d_src = torch.from_numpy(src).to(dev)
    d_noise = torch.from_numpy(padded(n, nslack)).to(dev)
    if in_place:
        out.copy_(d_src.flatten())
        d_src = out
    else:
        out.fill_(NAN)
    as_dev = lambda v: None if v is None else torch.tensor(list(v), dtype=torch.int64, device=dev)
    d_ratio = torch.from_numpy(np.asarray(ratio, dtype=np.float32)).to(dev)
    ctx.mix_device(d_src, out, d_noise, rows, C, n.shape[1], S, Sn, T, as_dev(valid), as_dev(nvalid), d_ratio,
                   stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert bool((torch.cat([raw[:GUARD], raw[GUARD + total:]]).view(torch.uint8) == 0x5A).all()), "a guard was written"
    got = out.cpu().numpy().reshape(rows, C, S)
    assert np.isnan(got[:, :, T:]).all(), "an element behind frames was written"
    back = d_noise.cpu().numpy()
    assert np.array_equal(back[:, :, :T], n, equal_nan=True) and np.isnan(back[:, :, T:]).all(), "the noise was written"
    if not in_place:
        back = d_src.cpu().numpy()
        assert np.array_equal(back[:, :, :T], x, equal_nan=True) and np.isnan(back[:, :, T:]).all(), "the source was written"
    return got[:, :, :T].copy()


REFS = {}


def reference(key, x, n, ratio, valid, nvalid):
    """(y, dY, twin) of an input, computed once per key and shared"""
    from alac.net_amd.mix import mix_host, mix_host_f32

    if key not in REFS:
        y, dY = mix_host(x, n, ratio, valid, nvalid, bound=True)
        t = mix_host_f32(x, n, ratio, valid, nvalid)
        for a in (y, dY, t):
            a.setflags(write=False)
        REFS[key] = (y, dY, t)
    return REFS[key]


def check(got, ref, tag):
    y, dY, t = ref
    fin = np.isfinite(y)
    assert same_bits(got.astype(np.float64)[~fin], y[~fin]), (tag, "where the specification is not finite the kernel must be that")
    err = np.where(fin, np.abs(got.astype(np.float64) - np.where(fin, y, 0.0)), 0.0)
    live = fin & (dY > 0)
    r_gpu = float(np.max(err[live] / dY[live])) if live.any() else 0.0
    r_twin = float(np.max(np.abs(t.astype(np.float64) - y)[live] / dY[live])) if live.any() else 0.0
    equal = same_bits(got, t)
    print(f"{tag}: max err {float(err.max()):.3e}, r_gpu {r_gpu:.5f}, r_twin {r_twin:.5f}, equal bits {equal}")
    assert (~fin | (err <= dY)).all(), (tag, int(np.argmax(np.where(fin, err - dY, -np.inf))), float(err.max()))
    assert r_gpu <= 4 * r_twin, (tag, r_gpu, r_twin)
    assert equal, (tag, "not the twin's bits", int(np.argmax(~((got == t) | (np.isnan(got) & np.isnan(t))))))


def lengths_for(T, rows, turn):
    """`rows` pairs (v, vn) out of full, partial, 0, -1, beyond T and noise shorter than the signal, another selection every turn"""
    pool = [(T, T), (T // 2, T), (T, max(T // 3, 1)), (T + 5, T + 5), (0, T), (max(T - 1, 0), max((2 * T) // 3, 1)), (T, 0), (-1, T),
            (T, 1), (T, -1), ((2 * T) // 3, T // 2), (1, T), (T, max(T - 1, 1))]
    picks = [pool[(turn + 4 * r) % len(pool)] for r in range(rows)]
    return [p[0] for p in picks], [p[1] for p in picks]


def small_frames():
    part, vec, rnd = constant("ALAC_MIX_PART"), constant("ALAC_MIX_VEC"), constant("ALAC_MIX_ROUND")
    assert constant("ALAC_MIX_THREADS") * vec == rnd and part % rnd == 0
    return sorted({1, 2, vec - 1, vec, vec + 1, rnd - 1, rnd, rnd + 1, part - 1, part, part + 1, 2 * part - 1, 2 * part, 2 * part + 1})


@pytest.mark.parametrize("T", small_frames())
def test_grid_of_frames_channels_and_layouts(gpu, T):
    """Three rows; frames one below, at and one above the vector width, a round, a part and two parts; C in 1, 2 and Cn in 1, C;
    planes off and at multiples of 16 bytes; out of place and in place"""
    turn = 5 * T
    for C, Cn in ((1, 1), (2, 1), (2, 2)):
        x, n = noise((3, C, T), 1000 + T + C), (0.3 * noise((3, Cn, T), 2000 + T + Cn)).astype(np.float32)
        ratio = np.random.default_rng(T + C + Cn).uniform(0.05, 2.0, 3).astype(np.float32)
        for k, (slack, nslack) in enumerate(((SLACK, SLACK), (wide(T), wide(T)), (wide(T), SLACK), (SLACK, wide(T)))):
            valid, nvalid = lengths_for(T, 3, turn)
            tag = f"T {T} C {C} Cn {Cn} slack {slack}/{nslack} valid {valid} noise valid {nvalid}"
            ref = reference((T, C, Cn, tuple(valid), tuple(nvalid)), x, n, ratio, valid, nvalid)
            check(run(gpu, x, n, ratio, valid, nvalid, slack, nslack, in_place=bool(k % 2)), ref, tag)
            turn += 1
        ref = reference((T, C, Cn, None), x, n, ratio, None, None)
        check(run(gpu, x, n, ratio), ref, f"T {T} C {C} Cn {Cn} whole")
        check(run(gpu, x, n, ratio, slack=wide(T), nslack=wide(T), in_place=True), ref, f"T {T} C {C} Cn {Cn} whole, 16 bytes, in place")


def large_frames():
    most = constant("ALAC_MIX_MAX_PARTS") * constant("ALAC_MIX_PART")
    return [most - 1, most, most + 1]


@pytest.mark.parametrize("T", large_frames())
def test_the_largest_part_count_and_the_first_longer_part(gpu, T):
    """ALAC_MIX_MAX_PARTS parts of ALAC_MIX_PART frames, and one frame more: parts of twice the length"""
    from alac.net_amd.mix import part_frames

    part, most = constant("ALAC_MIX_PART"), constant("ALAC_MIX_MAX_PARTS")
    assert part_frames(T) == (part if T <= part * most else 2 * part) and -(-T // part_frames(T)) == (most if T <= part * most else most // 2 + 1)
    x, n = noise((3, 1, T), T % 1000), (0.5 * noise((3, 1, T), T % 1000 + 1)).astype(np.float32)
    ratio = np.array([0.5, 1.5, 0.1], dtype=np.float32)
    valid, nvalid = [T, T - 12345, T], [T, T, 300001]
    ref = reference((T, "large"), x, n, ratio, valid, nvalid)
    for slack, in_place in ((SLACK, False), (wide(T), True)):
        check(run(gpu, x, n, ratio, valid, nvalid, slack, slack, in_place), ref, f"T {T} slack {slack} in place {in_place}")


def every_kind(T, C, Cn, seed):
    """Rows of every kind in one call: (x, n, ratio, valid, nvalid) and the index of each kind"""
    part = constant("ALAC_MIX_PART")
    kinds = ["full", "partial", "tiled", "v 0", "v -1", "vn 0", "vn -1", "a 0", "pn 0", "plain a", "plain b", "vn 1", "ps 0", "negative"]
    at = {k: i for i, k in enumerate(kinds)}
    B = len(kinds)
    x, n = noise((B, C, T), seed), (0.2 * noise((B, Cn, T), seed + 1)).astype(np.float32)
    ratio = np.random.default_rng(seed).uniform(0.1, 1.5, B).astype(np.float32)
    valid, nvalid = [T] * B, [T] * B
    valid[at["partial"]] = T - T // 3
    nvalid[at["tiled"]] = min(part - 96, T // 2) + 1          # the repeats do not line up with the parts
    valid[at["v 0"]], valid[at["v -1"]], nvalid[at["vn 0"]], nvalid[at["vn -1"]] = 0, -1, 0, -1
    ratio[at["a 0"]] = 0.0
    n[at["a 0"]] = np.nan
    n[at["pn 0"]] = 0.0
    nvalid[at["vn 1"]] = 1
    x[at["ps 0"]] = 0.0
    ratio[at["negative"]] *= -1
    valid[at["plain b"]], nvalid[at["plain b"]] = T - 10, T - 3
    return x, n, ratio, valid, nvalid, at


def kind_shapes():
    part = constant("ALAC_MIX_PART")
    return [(2 * part + 77, 2, 1), (part + 1000, 1, 1), (3001, 2, 2)]


@pytest.mark.parametrize("T,C,Cn", kind_shapes())
def test_rows_of_every_kind_in_one_call(gpu, T, C, Cn):
    x, n, ratio, valid, nvalid, at = every_kind(T, C, Cn, 77 + T)
    ref = reference((T, C, Cn, "kinds"), x, n, ratio, valid, nvalid)
    outs = []
    for slack, nslack, in_place in ((SLACK, SLACK, False), (wide(T), wide(T), False), (SLACK, wide(T), True), (wide(T), SLACK, True)):
        got = run(gpu, x, n, ratio, valid, nvalid, slack, nslack, in_place)
        check(got, ref, f"T {T} C {C} Cn {Cn} kinds, slack {slack}/{nslack}, in place {in_place}")
        outs.append(got)
    got = outs[0]
    for k in ("v 0", "v -1", "vn 0", "vn -1", "a 0", "pn 0", "ps 0"):          # x bit for bit
        assert np.array_equal(got[at[k]].view(np.int32), x[at[k]].view(np.int32)), k
    for k in ("full", "partial", "tiled", "plain a", "plain b", "vn 1", "negative"):
        assert not np.array_equal(got[at[k]], x[at[k]]) and np.isfinite(got[at[k]]).all(), k
    b = at["partial"]
    assert np.array_equal(got[b, :, valid[b]:].view(np.int32), x[b, :, valid[b]:].view(np.int32))
    # every row alone is the row of the batch
    for k in ("tiled", "plain b", "a 0"):
        b = at[k]
        alone = run(gpu, x[b:b + 1], n[b:b + 1], ratio[b:b + 1], valid[b:b + 1], nvalid[b:b + 1])
        assert same_bits(alone[0], got[b]), k


@pytest.mark.parametrize("T,C,Cn", kind_shapes()[:2])
def test_what_is_not_finite_stays_in_its_row(gpu, T, C, Cn):
    x, n, ratio, valid, nvalid, at = every_kind(T, C, Cn, 77 + T)
    ref = run(gpu, x, n, ratio, valid, nvalid)
    a, b = at["plain a"], at["plain b"]
    others = [r for r in range(len(at)) if r not in (a, b)]
    for bad in (np.nan, np.inf):
        z, m = x.copy(), n.copy()
        z[a, C - 1, T // 3] = bad                      # inside v of one row's signal
        m[b, 0, nvalid[b] - 1] = bad                   # inside vn of another row's noise, behind its v
        for in_place in (False, True):
            got = run(gpu, z, m, ratio, valid, nvalid, in_place=in_place)
            assert same_bits(got[others], ref[others]), (bad, in_place, "another row changed")
            if np.isnan(bad):
                assert np.isnan(got[a]).all() and np.isnan(got[b, :, :valid[b]]).all(), bad
            else:                                      # Ps = inf: g = inf; Pn = inf: Ps / inf = 0 = g, the row stays
                assert not np.isfinite(got[a]).any() and same_bits(got[b], x[b]), bad
            assert same_bits(got[b, :, valid[b]:], x[b, :, valid[b]:])
        check(got, reference((T, C, Cn, "bad", str(bad)), z, m, ratio, valid, nvalid), f"T {T} with {bad}")
    # at or behind v and vn, and in a row that gets no noise: never read
    z, m = x.copy(), n.copy()
    p, t = at["partial"], at["tiled"]
    m[t, :, nvalid[t]:] = np.nan
    m[b, :, nvalid[b]:] = np.inf
    m[at["v 0"]] = m[at["v -1"]] = np.nan
    z[at["v 0"]] = z[at["v -1"]] = np.nan
    z[p, :, valid[p]:] = np.nan
    for in_place in (False, True):
        got = run(gpu, z, m, ratio, valid, nvalid, in_place=in_place)
        want = ref.copy()
        want[at["v 0"]] = want[at["v -1"]] = np.nan    # (x itself)
        want[p, :, valid[p]:] = np.nan
        assert same_bits(got, want), in_place


def test_the_public_call(gpu):
    import alac.net_amd as pkg
    from alac.net_amd.mix import mix_host_f32, snr_ratio

    torch, _ = gpu
    B, C, T = 4, 2, 5000
    x, n = noise((B, C, T), 5), (0.1 * noise((B, 1, T), 6)).astype(np.float32)
    d, dn = torch.from_numpy(x).cuda(), torch.from_numpy(n).cuda()
    snr = [10.0, NAN, 0.0, 25.5]
    lengths, nlen = [T, 4000, -1, 3000], [T, T, T, 1234]
    ratio = snr_ratio(snr, B, d.device).cpu().numpy()
    assert ratio.dtype == np.float32 and ratio[1] == 0 and ratio[2] == 1 and abs(ratio[0] - 10 ** -0.5) < 1e-6
    want = mix_host_f32(x, n, ratio, lengths, nlen)
    got = pkg.mix(d, dn, snr, lengths, nlen)
    assert got.shape == d.shape and got.data_ptr() != d.data_ptr() and torch.equal(d.cpu(), torch.from_numpy(x))
    assert same_bits(got.cpu().numpy(), want)
    assert np.array_equal(want[1], x[1]) and np.array_equal(want[2], x[2]) and not np.array_equal(want[0], x[0])
    for s in (torch.tensor(snr), torch.tensor(snr, device="cuda"), np.array(snr), torch.tensor(snr, dtype=torch.float64)):
        assert torch.equal(pkg.mix(d, dn, s, torch.tensor(lengths, device="cuda"), torch.tensor(nlen, dtype=torch.int32)).view(torch.int32),
                           got.view(torch.int32))
    e = d.clone()
    assert pkg.mix(e, dn, snr, lengths, nlen, out=e) is e and torch.equal(e.view(torch.int32), got.view(torch.int32))
    # one number for every row, and whole rows
    assert same_bits(pkg.mix(d, dn, 6.0).cpu().numpy(), mix_host_f32(x, n, snr_ratio(6.0, B, d.device).cpu().numpy()))
    # the slice [..., :T - 1] of both: the last column is neither read nor written
    z, m = x.copy(), n.copy()
    z[..., -1] = m[..., -1] = np.nan
    dz, dm = torch.from_numpy(z).cuda(), torch.from_numpy(m).cuda()
    want = mix_host_f32(np.ascontiguousarray(x[..., :-1]), np.ascontiguousarray(n[..., :-1]), ratio, lengths, nlen)
    assert same_bits(pkg.mix(dz[..., :-1], dm[..., :-1], snr, lengths, nlen).cpu().numpy(), want)
    assert pkg.mix(dz[..., :-1], dm[..., :-1], snr, lengths, nlen, out=dz[..., :-1]).data_ptr() == dz.data_ptr()
    back = dz.cpu().numpy()
    assert same_bits(back[..., :-1], want) and np.isnan(back[..., -1]).all()
    assert pkg.mix(d[:0], dn[:0], 3.0).shape == (0, C, T)
    # ValueError before any device work
    for args in ((d.cpu(), dn, 10.0), (d, dn.cpu(), 10.0), (d.double(), dn, 10.0), (d, dn.double(), 10.0), (d[0], dn[0], 10.0),
                 (d, dn[:2], 10.0), (d, dn[..., :-1], 10.0), (d, torch.zeros(B, 3, T, device="cuda"), 10.0), (d[..., ::2], dn[..., ::2], 10.0),
                 (d, dn, [1.0, 2.0]), (d, dn, "loud"), (d, dn, torch.ones(B + 1)), (d, dn, 10.0, [1, 2]), (d, dn, 10.0, [1.0] * B),
                 (d, dn, 10.0, None, torch.ones(B, device="cuda")), (d, d, 10.0, None, None, d)):
        with pytest.raises(ValueError):
            pkg.mix(*args)
    for out in (d[..., :-1], d.double(), d.cpu(), torch.empty(B, C, T + 1, device="cuda")[..., :T], dn.expand(B, C, T)):
        with pytest.raises(ValueError):
            pkg.mix(d, dn, 10.0, out=out)


def test_bad_arguments_are_refused_and_nothing_is_enqueued(gpu):
    import alac.net_amd as pkg

    torch, ctx = gpu
    rows, C, S, T = 3, 2, 16, 10
    src = torch.zeros(rows * C * S + 8, device="cuda")
    out = torch.full((rows * C * S + 8,), 7.0, device="cuda")
    nse = torch.ones(rows * S + 8, device="cuda")
    valid, nvalid = torch.full((rows + 1,), T, dtype=torch.int64, device="cuda"), torch.full((rows + 1,), T, dtype=torch.int64, device="cuda")
    ratio = torch.ones(rows + 1, device="cuda")
    base = dict(d_src=src.data_ptr(), d_out=out.data_ptr(), d_noise=nse.data_ptr(), rows=rows, channels=C, noise_channels=1, stride=S,
                noise_stride=S, frames=T, d_valid=valid.data_ptr(), d_noise_valid=nvalid.data_ptr(), d_ratio=ratio.data_ptr(), stream=None)
    extent = 4 * ((rows * C - 1) * S + T)
    far = 1 << 44
    cases = [dict(d_src=None), dict(d_out=None), dict(d_noise=None), dict(d_ratio=None), dict(d_src=base["d_src"] + 2),
             dict(d_out=base["d_out"] + 2), dict(d_noise=base["d_noise"] + 1), dict(d_ratio=base["d_ratio"] + 2),
             dict(d_valid=base["d_valid"] + 4), dict(d_noise_valid=base["d_noise_valid"] + 4), dict(channels=0), dict(noise_channels=0),
             dict(noise_channels=3), dict(frames=0), dict(frames=S + 1), dict(stride=T - 1), dict(noise_stride=T - 1),
             dict(d_out=base["d_src"] + 4), dict(d_out=base["d_src"] + extent - 4), dict(d_noise=base["d_out"]),
             dict(d_noise=base["d_out"] + extent - 4), dict(d_out=base["d_src"], d_noise=base["d_src"] + 16),
             dict(stride=1 << 58), dict(noise_stride=1 << 58),
             dict(d_out=base["d_src"], d_noise=base["d_src"] + far, rows=1 << 31, channels=1, stride=1, noise_stride=1, frames=1)]
    fn = pkg.lib().alacgpu_mix_device
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
    assert bool((got[:, :, :T] == 0).all()) and bool((got[:, :, T:] == 7.0).all())      # Ps == 0: g = 0, the copy of x
