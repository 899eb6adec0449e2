"""alacgpu_resample_ratio_rows_device alone: one batch [8, 2, 3000] whose rows have ratios and windows of their own, against the
float64 specification within the stated bound, against the float32 twin bit for bit (the twin's fused multiply-adds are
exact), and the entry's refusals."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

T, OUT = 3000, 701
SENTINEL = 12345.0
# (a, b, valid, out_first); a == 0: the row is skipped
ROWS = [(9, 10, T, 0), (11, 10, T, 0), (3969, 1600, T, 0), (33, 5, T, 0), (3969, 1600, T, -5), (9, 10, 0, 0),
        (11, 10, 1234, -(-10 * 1234 // 11) - 300), (0, 1, T, 0)]


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def batch():
    """The source on the host and the device, the call's ratios and, per (mono, out_frames), the references made once"""
    import torch

    from alac.net_amd.resample import filter_width

    rng = np.random.default_rng(77)
    t = np.arange(T) / 44100.0
    x = np.stack([np.stack([0.3 * np.sin(2 * np.pi * (300 + 170 * r) * t + c) + 0.05 * rng.standard_normal(T) for c in (0, 1)])
                  for r in range(len(ROWS))]).astype(np.float32)
    ratios, row_ratio = [], []
    for a, b, _, _ in ROWS:
        d = (a, b, filter_width(a, b) if a else 0)
        if d not in ratios:
            ratios.append(d)
        row_ratio.append(ratios.index(d))
    up = lambda v, dt: torch.from_numpy(np.asarray(v, dtype=dt)).to("cuda")
    dev = dict(src=torch.from_numpy(x).to("cuda"), origin=torch.zeros(len(ROWS), dtype=torch.int64, device="cuda"),
               valid=up([r[2] for r in ROWS], np.int64), first=up([r[3] for r in ROWS], np.int64),
               ratios=np.asarray(ratios, dtype=np.uint32), d_ratios=up(np.asarray(ratios, dtype=np.uint32).view(np.int32), np.int32),
               row_ratio=up(row_ratio, np.int32))
    return x, dev, {}


def references(batch, mono, frames):
    from alac.net_amd.resample import filter_width
    from alac.net_amd.speed import speed_bound, speed_host, speed_host_f32

    x, _, cache = batch
    if (mono, frames) not in cache:
        want, tol, twin = [], [], []
        for r, (a, b, valid, first) in enumerate(ROWS):
            if a == 0:
                shape = (1 if mono else 2, frames)
                want.append(np.full(shape, SENTINEL)), tol.append(np.zeros(shape)), twin.append(np.full(shape, SENTINEL, np.float32))
                continue
            kw = dict(mono=mono, first=first, num_frames=frames)
            xr, w = x[r, :, :valid], filter_width(a, b)
            want.append(speed_host(xr.astype(np.float64), a, b, w, **kw))
            tol.append(speed_bound(xr.astype(np.float64), a, b, w, **kw))
            twin.append(speed_host_f32(xr, a, b, w, **kw))
        cache[mono, frames] = np.stack(want), np.stack(tol), np.stack(twin)
    return cache[mono, frames]


def call(dev, mono, frames, out=None, **over):
    import torch

    from alac.net_amd.resample import _context

    a = dict(dev, **over)
    if out is None:
        out = torch.full((len(ROWS), 1 if mono else 2, frames), SENTINEL, dtype=torch.float32, device="cuda")
    _context(0).resample_ratio_rows_device(a["src"], a.get("rows", len(ROWS)), a.get("channels", 2), T, a["origin"], a["valid"], a["first"],
                                           frames, a["ratios"], a["d_ratios"], a["row_ratio"], mono, out,
                                           stream=torch.cuda.current_stream().cuda_stream)
    return out


@pytest.mark.parametrize("mono", [False, True])
def test_rows_equal_the_specification_and_the_twin(batch, mono):
    x, dev, _ = batch
    want, tol, twin = references(batch, mono, OUT)
    out = call(dev, mono, OUT)
    got = out.cpu().numpy()
    err = np.abs(got.astype(np.float64) - want)
    print(f"mono={mono}: worst err / bound {float((err / np.maximum(tol, 1e-300))[:7].max()):.3f}, "
          f"{int((bits(got) != bits(twin)).sum())} elements differ from the twin")
    assert (err <= tol).all(), [float((err[r] / np.maximum(tol[r], 1e-300)).max()) for r in range(len(ROWS))]
    assert not got[want == 0].any()                                            # zeros where the specification has zeros
    assert not got[3, :, -(-5 * T // 33):].any() and not got[4, :, :5].any() and not got[5].any() and not got[6, :, 300:].any()
    assert got[6, :, :300].all() and got[0].any() and got[2].any()
    assert (got[7] == SENTINEL).all()                                          # the skipped row is untouched
    assert np.array_equal(bits(got), bits(twin))
    assert np.array_equal(bits(call(dev, mono, OUT).cpu().numpy()), bits(got))   # the same call, the same bits


def test_a_workgroup_that_runs_several_tiles(batch):
    """2^17 + 77 output frames of 16 planes: more than 2048 tiles, so a workgroup takes two; the signal ends within the first
    4000 frames, which are compared with the twin, and everything behind is zero"""
    x, dev, _ = batch
    frames, head = (1 << 17) + 77, 4000
    want, tol, twin = references(batch, False, head)
    got = call(dev, False, frames).cpu().numpy()
    assert np.array_equal(bits(got[:, :, :head]), bits(twin))
    assert (np.abs(got[:, :, :head].astype(np.float64) - want) <= tol).all()
    assert not got[:7, :, head:].any() and (got[7] == SENTINEL).all()


def test_refusals_launch_nothing(batch):
    import torch

    import alac.net_amd as pkg

    x, dev, _ = batch
    out = torch.full((len(ROWS), 2, OUT), SENTINEL, dtype=torch.float32, device="cuda")

    def with_ratio(i, triple):
        r = dev["ratios"].copy()
        r[i] = triple
        return dict(ratios=r, d_ratios=torch.from_numpy(r.view(np.int32)).to("cuda"))

    bad = [with_ratio(0, (9, 0, 7)), with_ratio(4, (0, 0, 0)), with_ratio(1, (1 << 31, 10, 7)), with_ratio(1, (11, 1 << 31, 7)),
           with_ratio(2, (3969, 1600, 0)), with_ratio(3, (33, 5, 20480)), dict(ratios=np.zeros((0, 3), np.uint32)), dict(channels=3),
           dict(d_ratios=None), dict(row_ratio=None), dict(src=None)]
    for over in bad:
        with pytest.raises(pkg.AlacGpuError, match="bad argument|BAD_ARG|invalid"):
            call(dev, False, OUT, out=out, **over)
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()


def test_speed_perturb_on_a_batch(batch):
    """alac.speed_perturb: a factor per row, lengths, the copy at factor 1 and equal rates, zeros behind the new lengths"""
    import torch

    import alac.net_amd as pkg
    from alac.net_amd.speed import ratio, speed_host_f32

    x, dev, _ = batch
    lens = [T, 2500, 1234, T]
    factors = [0.9, 1, 1.1, 1.1]
    for mono in (False, True):
        y, new = pkg.speed_perturb(dev["src"][:4], factors, 16000, lengths=lens, mono=mono)
        assert new.tolist() == [-(-10 * T // 9), 2500, -(-10 * 1234 // 11), -(-10 * T // 11)] and y.shape == (4, 1 if mono else 2, -(-10 * T // 9))
        got = y.cpu().numpy()
        for r, f in enumerate(factors):
            n = int(new[r])
            if f == 1:
                src = x[r, :, :n] if not mono else (x[r, 0:1, :n] + x[r, 1:2, :n]) * np.float32(0.5)
                assert np.array_equal(bits(got[r, :, :n]), bits(src))               # a copy, bit for bit
            else:
                twin = speed_host_f32(x[r, :, :lens[r]], *ratio(16000, f, 16000), mono=mono)
                assert twin.shape[1] == n and np.array_equal(bits(got[r, :, :n]), bits(twin))
            assert not got[r, :, n:].any()
    one, one_len = pkg.speed_perturb(dev["src"][:2], 1.1, 44100, 16000)
    a, b, w = ratio(44100, 1.1, 16000)
    assert one.shape == (2, 2, -(-b * T // a)) and one_len.tolist() == [one.shape[2]] * 2
    assert np.array_equal(bits(one[1].cpu().numpy()), bits(speed_host_f32(x[1], a, b, w)))
    for bad in (dict(factors=[0.9]), dict(factors=3.0), dict(lengths=[1.0, 2.0])):
        with pytest.raises(ValueError):
            pkg.speed_perturb(dev["src"][:2], **dict(dict(factors=1.1, orig_rate=16000), **bad))


# (a, b, valid, out_first, origin): ratios whose integers need 64 bits -- 1200 * max(a, b) is 2^31 and more -- next to one that does not
WIDE = [(1999993, 2000003, 1200, 0, 0), (1999993, 2000003, 1200, -5, 0), (2000003, 1999993, 1200, 0, 0),
        (1999993, 2000003, 1200, 1000003, 999992), (9, 10, 1200, 0, 0)]


def test_ratios_that_need_64_bit_integers():
    """The kernel's 64-bit instantiation: [5, 2, 1200] into 1101 frames, two tiles a plane and the second one partial.  Coprime
    ratios near 1 of two million a side, one with leading zeros (taps that must not wrap), one with a > b, one whose j * a is
    far above 2^32, and a row at 9 : 10 that takes the 32-bit instantiation in the same launch.  Bit for bit the float32 twin,
    which evaluates only the phases used (the specification's table would have 30 million weights); the twin's weights of those
    phases within EPS_W * scale of resample.py's closed form in float64; zeros where the twin has zeros; and a row whose ratio
    is skipped keeps its sentinel."""
    import torch

    from alac.net_amd.resample import ROLLOFF, ZERO_CROSSINGS, _context, filter_width
    from alac.net_amd.speed import EPS_W, speed_host_f32, weights_f32

    n, frames = 1200, 1101
    rng = np.random.default_rng(78)
    t = np.arange(n) / 44100.0
    x = np.stack([np.stack([0.3 * np.sin(2 * np.pi * (300 + 170 * r) * t + c) + 0.05 * rng.standard_normal(n) for c in (0, 1)])
                  for r in range(len(WIDE))]).astype(np.float32)
    assert all(filter_width(a, b) == 7 for a, b, *_ in WIDE)
    # the weights of the phases used against the closed form: t = f (d b - r) / (a b), w = (f / a) sinc(t) cos^2(pi t / 12)
    d = np.arange(-7, 8, dtype=np.int64)
    for a, b, _, first, _ in WIDE:
        assert (1200 * max(a, b) >= 1 << 31) == (a != 9)
        phases = np.unique(((first + np.arange(frames, dtype=np.int64)) * a) % b)
        f = ROLLOFF * min(a, b)
        u = f * ((d[None, :] * b - phases[:, None]).astype(np.float64) / (a * b))
        w64 = np.where(np.abs(u) < ZERO_CROSSINGS, (f / a) * np.sinc(u) * np.cos(np.pi * u / (2 * ZERO_CROSSINGS)) ** 2, 0.0)
        err = np.abs(weights_f32(a, b, 7, phases).astype(np.float64) - w64).max() / (f / a)
        print(f"{a} : {b} from {first}: weights within {err * 2 ** 24:.1f} units of 2^-24 of the closed form")
        assert err <= EPS_W
    ratios = np.array([(1999993, 2000003, 7), (2000003, 1999993, 7), (9, 10, 7)], dtype=np.uint32)
    up = lambda v, dt: torch.from_numpy(np.asarray(v, dtype=dt)).to("cuda")
    src, d_ratios = torch.from_numpy(x).to("cuda"), up(ratios.view(np.int32), np.int32)
    valid, first, origin = (up([r[k] for r in WIDE], np.int64) for k in (2, 3, 4))
    for mono in (False, True):
        twin = np.stack([speed_host_f32(x[r, :, :v], a, b, 7, mono=mono, origin=o, first=j, num_frames=frames)
                         for r, (a, b, v, j, o) in enumerate(WIDE)])
        got = {}
        for skipped in (None, 3):
            row_ratio = [0, 0, 1, 0, 2]
            if skipped is not None:
                row_ratio[skipped] = len(ratios)
            out = torch.full((len(WIDE), 1 if mono else 2, frames), SENTINEL, dtype=torch.float32, device="cuda")
            _context(0).resample_ratio_rows_device(src, len(WIDE), 2, n, origin, valid, first, frames, ratios, d_ratios,
                                                   up(row_ratio, np.int32), mono, out, stream=torch.cuda.current_stream().cuda_stream)
            got[skipped] = out.cpu().numpy()
        assert np.array_equal(bits(got[None]), bits(twin)), [int((bits(got[None][r]) != bits(twin[r])).sum()) for r in range(len(WIDE))]
        assert not got[None][twin == 0].any() and not got[None][1, :, :5].any() and all(got[None][r].any() for r in range(len(WIDE)))
        assert (got[3][3] == SENTINEL).all() and np.array_equal(bits(np.delete(got[3], 3, 0)), bits(np.delete(twin, 3, 0)))
