"""alac.net_amd/rir.py without a device: the image-source specification against figures worked out by hand and with a numpy
model (the direct path, the image counts, reciprocity, the decay against Sabine), the float32 twin against the specification
within the derived bound, the refusals, and the arguments of `ShoeboxRooms` and `Reverb`."""
import math
import os
import re

import numpy as np
import pytest

import alac.net_amd as pkg
from alac.net_amd import rir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOM = [3.0, 2.5, 2.0, 1.1, 0.9, 1.2, 2.0, 1.7, 0.8]


def geom(*rows):
    return np.array(rows, dtype=np.float64).reshape(-1, 9)


def betas(rows, value):
    return np.full((rows, 6), value, dtype=np.float32)


def test_direct_path_is_one_tap_of_one_over_4_pi_d():
    d = 343.0 * 20 / 8000
    g = geom([4, 3, 2.5, 1, 1, 1, 1 + d, 1, 1])
    h, lengths, bound = rir.rir_host(g, betas(1, 0.0), 8000, 200, bound=True)
    assert lengths.tolist() == [200] and h.shape == (1, 1, 200)
    assert abs(h[0, 0, 20] - 1 / (4 * math.pi * d)) < 1e-12 and abs(h[0, 0, 20] - 0.0928017) < 1e-7
    assert np.abs(np.delete(h[0, 0], 20)).max() < 1e-15
    h32, l32 = rir.rir_host_f32(g, betas(1, 0.0), 8000, 200)
    assert l32.tolist() == [200] and h32.dtype == np.float32
    assert (np.abs(h32 - h) <= bound).all()
    assert rir.image_counts(g[0], 8000, 200, max_order=0)[0] == 1


def test_image_counts():
    for order, images in ((0, 1), (1, 7), (2, 25), (3, 63)):
        assert rir.image_counts(ROOM, 8000, 600, max_order=order)[0] == images
        # ... and as the sum of a response whose walls reflect everything: every image adds 1 / (4 pi d) > 0 at its own taps
    assert rir.image_counts(ROOM, 8000, 600) == (5748, 29640)
    h, _ = rir.rir_host(geom(ROOM), betas(1, 0.8), 8000, 600)
    assert int(np.argmax(np.abs(h[0, 0]))) == 30


def test_reciprocity():
    g = geom(ROOM)
    swapped = geom(ROOM[:3] + ROOM[6:] + ROOM[3:6])
    a, _, da = rir.rir_host(g, betas(1, 0.8), 8000, 600, bound=True)
    b, _, db = rir.rir_host(swapped, betas(1, 0.8), 8000, 600, bound=True)
    print("reciprocity:", np.abs(a - b).max())
    assert np.abs(a - b).max() <= 1e-15
    a32, _ = rir.rir_host_f32(g, betas(1, 0.8), 8000, 600)
    b32, _ = rir.rir_host_f32(swapped, betas(1, 0.8), 8000, 600)
    assert (np.abs(a32 - b32) <= da + db).all()


GRID = [(ROOM, [0.8] * 6, 600, 81, None), (ROOM, [0.9, 0.5, 0.7, 0.95, 0.3, 0.6], 300, 41, None), (ROOM, [1.0] * 6, 200, 3, None),
        (ROOM, [0.8] * 6, 600, 81, 3), ([4, 3, 2.5, 1, 1, 1, 1 + 343.0 * 20 / 8000, 1, 1], [0.0] * 6, 200, 81, None),
        ([5, 4, 3, 2.5, 2, 1.5, 2.55, 2, 1.5], [0.7] * 6, 150, 81, None)]


def test_twin_is_within_the_bound_and_the_bound_is_not_vacuous():
    closest = 0.0
    for g, b, K, W, order in GRID:
        g, b = geom(g), np.array([b], dtype=np.float32)
        h, _, bound = rir.rir_host(g, b, 8000, K, taps=W, max_order=order, bound=True)
        h32, _ = rir.rir_host_f32(g, b, 8000, K, taps=W, max_order=order)
        err = np.abs(h32 - h)
        assert (err <= bound).all(), (K, W, order, (err / np.maximum(bound, 1e-300)).max())
        closest = max(closest, (err[bound > 0] / bound[bound > 0]).max())
    print("closest to the bound:", closest)
    assert closest >= 1e-3


def test_the_twin_sums_a_tap_in_image_order():
    """np.add.at in `rir_host_f32` against a loop over the images, one float32 addition at a time"""
    g, b = geom(ROOM), betas(1, 0.8)
    h32, _ = rir.rir_host_f32(g, b, 8000, 100, taps=41)
    H, scale = 20, 8000 / 343.0
    N = rir.candidate_box(g[0], scale, 100, H, -1)
    n, p, d, tau, k0, f = rir._images(g[0], scale, 100, H, -1, N)
    cw, sw, TW = rir.window_table(41)
    f32 = np.float32
    row = np.zeros(100, dtype=f32)
    for i in range(len(d)):
        e = rir._exponents(n[i:i + 1], p[i:i + 1])
        pw = rir._pow_f32(np.full((1, 6), 0.8, dtype=f32), e)[0]
        A = f32(((pw[0] * pw[1]) * (pw[2] * pw[3])) * (pw[4] * pw[5])) / f32(rir._FOUR_PI * d[i])
        ff = f32(f[i])
        sp, cphi, sphi = rir._sin_poly(rir._PI * ff), rir._cos_poly(TW * ff), rir._sin_poly(TW * ff)
        for m in range(-H, H + 1):
            k = int(k0[i]) + m
            if 0 <= k < 100:
                c = f32(cw[abs(m)] * cphi) + f32((-sw[-m] if m < 0 else sw[m]) * sphi)
                w = f32(0.5) + f32(f32(0.5) * c)
                tt = f32(m) - ff
                s = f32(1) if tt == 0 else f32((sp if m & 1 else -sp) / f32(rir._PI * tt))
                row[k] = row[k] + f32(A * f32(w * s))
    assert np.array_equal(row.view(np.int32), h32[0, 0].view(np.int32))


def t20(h, fs):
    edc = np.cumsum((h * h)[::-1])[::-1]
    db = 10 * np.log10(edc / edc[0])
    return 3.0 * (np.argmax(db <= -25.0) - np.argmax(db <= -5.0)) / fs


def decay(L, alpha):
    V, S = L[0] * L[1] * L[2], 2 * (L[0] * L[1] + L[0] * L[2] + L[1] * L[2])
    sabine = 0.161 * V / (S * alpha)
    K = int(round(min(1.2 * sabine, 0.6) * 8000))
    g = geom(list(L) + [0.3 * L[0], 0.4 * L[1], 0.45 * L[2], 0.7 * L[0], 0.55 * L[1], 0.5 * L[2]])
    h, _ = rir.rir_host(g, betas(1, math.sqrt(1 - alpha)), 8000, K)
    return t20(h[0, 0], 8000.0), sabine


@pytest.mark.parametrize("L,alpha", [((6, 5, 3), 0.3), ((4, 3.5, 2.5), 0.5), ((8, 6, 3.5), 0.2)])
def test_decay_against_sabine(L, alpha):
    t, sabine = decay(L, alpha)
    print("T20 / Sabine:", t / sabine)
    assert 0.8 <= t / sabine <= 2.0


def test_decay_shortens_as_absorption_rises():
    assert decay((4, 3.5, 2.5), 0.3)[0] > decay((4, 3.5, 2.5), 0.5)[0] > decay((4, 3.5, 2.5), 0.7)[0]


def test_refused_rows_are_zero_and_of_length_0():
    bad = [ROOM[:3] + [float("nan")] + ROOM[4:], [float("inf")] + ROOM[1:], [3.0, 0.0, 2.0] + ROOM[3:], [3.0, -2.5, 2.0] + ROOM[3:],
           ROOM[:3] + [3.1] + ROOM[4:], ROOM[:6] + [2.0, 1.7, -0.1], [1e-5, 2.5, 2.0, 5e-6, 0.9, 1.2, 5e-6, 1.7, 0.8], [1e-9, 2.5, 2.0, 5e-10, 0.9, 1.2, 5e-10, 1.7, 0.8]]
    g = geom(ROOM, *bad, ROOM)
    for fn in (rir.rir_host, rir.rir_host_f32):
        h, lengths = fn(g, betas(len(g), 0.8), 8000, 100)
        assert lengths.tolist() == [100] + [0] * len(bad) + [100]
        assert not h[1:-1].any() and h[0].any() and np.array_equal(h[0], h[-1])
    assert rir.image_counts(bad[-1], 8000, 100) == (0, 0)
    # the limit lets a 3 x 3 x 2.5 m room at 0.5 s and 16 kHz pass, and the smallest room of Ko et al.'s small range
    assert rir.candidate_box([3, 3, 2.5, 1, 1, 1, 2, 2, 2], 16000 / 343.0, 8000, 40, -1) == (30, 30, 36)
    assert rir.candidate_box([1, 1, 2, 0.5, 0.5, 1, 0.5, 0.5, 1], 16000 / 343.0, 8000, 40, -1) is not None
    assert rir.candidate_box([1, 1, 2, 0.5, 0.5, 1, 0.5, 0.5, 1], 16000 / 343.0, 16000, 40, -1) is None
    # a room so large that nothing arrives: zeros of full length
    far = geom([400, 400, 50, 10, 10, 10, 300, 300, 10])
    h, lengths = rir.rir_host_f32(far, betas(1, 0.8), 8000, 100)
    assert lengths.tolist() == [100] and not h.any()


def test_host_arguments():
    g, b = geom(ROOM), betas(1, 0.8)
    for bad in (dict(taps=80), dict(taps=1), dict(taps=129), dict(max_order=-1), dict(sound_speed=0.0), dict(sound_speed=float("nan"))):
        with pytest.raises(ValueError):
            rir.rir_host(g, b, 8000, 100, **bad)
    for fs, K in ((0, 100), (8000, 0), (8000.0, 100), (8000, rir.MAX_FRAMES + 1)):
        with pytest.raises(ValueError):
            rir.rir_host_f32(g, b, fs, K)
    with pytest.raises(ValueError):
        rir.rir_host(g.astype(np.float32), b, 8000, 100)
    with pytest.raises(ValueError):
        rir.rir_host(g, betas(2, 0.8), 8000, 100)


def test_shoebox_rooms_arguments_and_draws():
    import torch

    rooms = pkg.ShoeboxRooms()
    assert rooms == pkg.ShoeboxRooms() and hash(rooms) == hash(pkg.ShoeboxRooms()) and rooms.taps == 81 and rooms.max_order is None
    with pytest.raises(AttributeError):
        rooms.taps = 3
    for bad in (dict(room=((3, 10), (3, 10))), dict(room=((0, 10), (3, 10), (2, 3))), dict(room=((5, 4), (3, 10), (2, 3))),
                dict(absorption=None), dict(rt60=(0.3, 0.6)), dict(absorption=(0.2, 1.2)), dict(absorption=None, rt60=(0.0, 1.0)),
                dict(margin=2.0), dict(margin=-0.1), dict(taps=80), dict(max_order=-2), dict(sound_speed=0)):
        with pytest.raises(ValueError):
            pkg.ShoeboxRooms(**bad)
    with pytest.raises(ValueError):
        pkg.ShoeboxRooms.kaldi("huge")
    assert pkg.ShoeboxRooms.kaldi("small").room == ((1.0, 10.0), (1.0, 10.0), (2.0, 5.0))
    assert pkg.ShoeboxRooms.kaldi("large", margin=1.0).room[0] == (30.0, 50.0)

    def gen(seed):
        return torch.Generator().manual_seed(seed)

    a, b = rooms.draw(5, generator=gen(3)), rooms.draw(5, generator=gen(3))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    geometry, beta = a
    assert geometry.shape == (5, 9) and geometry.dtype == torch.float64 and beta.shape == (5, 6) and beta.dtype == torch.float32
    # the stated draws: 3 B, B, 3 B and 3 B float64 values, in this order
    g = gen(3)
    u = [torch.rand(shape, generator=g, dtype=torch.float64) for shape in ((5, 3), (5,), (5, 3), (5, 3))]
    lo, hi = torch.tensor([3.0, 3.0, 2.5], dtype=torch.float64), torch.tensor([10.0, 10.0, 4.0], dtype=torch.float64)
    L = lo + (hi - lo) * u[0]
    assert torch.equal(geometry[:, :3], L) and torch.equal(geometry[:, 3:6], 0.5 + (L - 1.0) * u[2])
    assert torch.equal(geometry[:, 6:], 0.5 + (L - 1.0) * u[3])
    assert torch.equal(beta, torch.sqrt(1.0 - (0.2 + 0.6 * u[1])).float()[:, None].expand(5, 6))
    after = torch.rand(1, generator=g, dtype=torch.float64)
    g2 = gen(3)
    rooms.draw(5, generator=g2)
    assert torch.equal(after, torch.rand(1, generator=g2, dtype=torch.float64))
    assert bool(((geometry[:, 3:6] >= 0.5) & (geometry[:, 3:6] <= L - 0.5)).all())
    # Sabine: alpha = 0.161 V / (S rt60), clipped
    geometry, beta = pkg.ShoeboxRooms(absorption=None, rt60=(0.4, 0.4)).draw(4, generator=gen(1))
    L = geometry[:, :3]
    V, S = L.prod(dim=1), 2 * (L[:, 0] * L[:, 1] + L[:, 0] * L[:, 2] + L[:, 1] * L[:, 2])
    assert torch.equal(beta[:, 0], torch.sqrt(1.0 - (0.161 * V / (S * 0.4)).clamp(0.01, 0.99)).float())


def test_reverb_over_rooms_arguments_and_draws():
    import torch

    rooms = pkg.ShoeboxRooms()
    aug = pkg.Reverb(rooms, p=0.5, max_seconds=0.5)
    assert aug.rooms is rooms and aug.frames(16000) == 8000 and aug == pkg.Reverb(rooms, 0.5, 0.5)
    for bad in (dict(p=1.5), dict(max_seconds=0.0)):
        with pytest.raises(ValueError):
            pkg.Reverb(rooms, **bad)
    with pytest.raises(ValueError):
        pkg.Reverb("rooms")
    with pytest.raises(ValueError, match="candidate images"):
        pkg.Reverb(pkg.ShoeboxRooms.kaldi("small"), max_seconds=1.0)
    pkg.Reverb(pkg.ShoeboxRooms.kaldi("small"), max_seconds=0.5).check_rate(16000)
    with pytest.raises(ValueError, match="candidate images"):
        pkg.Reverb(pkg.ShoeboxRooms(room=((0.8, 2), (0.8, 2), (2.0, 3)), margin=0.1), max_seconds=0.5).check_rate(16000)
    g = torch.Generator().manual_seed(5)
    geometry, beta, keep = aug.draw(7, generator=g, device="cpu")
    g = torch.Generator().manual_seed(5)
    want = rooms.draw(7, generator=g)
    assert torch.equal(geometry, want[0]) and torch.equal(beta, want[1])
    assert torch.equal(keep, torch.rand(7, generator=g, dtype=torch.float64) < 0.5)
    with pytest.raises(ValueError):
        aug.draw(7)


def test_the_call_is_declared_and_bound_alike():
    header = open(os.path.join(ROOT, "include", "alacgpu.h")).read()
    cs = open(os.path.join(ROOT, "alac.net_amd", "host", "csharp", "AlacGpuNative.cs")).read()
    m = re.search(r"int\s+alacgpu_rir_shoebox_device\s*\(([^)]*)\)", header)
    assert m and len(m.group(1).split(",")) == 13
    m = re.search(r"alacgpu_rir_shoebox_device\s*\(([^)]*)\)", cs)
    assert m and len(m.group(1).split(",")) == 13
    assert len(pkg.SYMBOLS["alacgpu_rir_shoebox_device"][1]) == 13
    h = open(os.path.join(ROOT, "alac.net_amd", "csrc", "alac_rir.h")).read()
    assert f"ALAC_RIR_LIMIT = {float(rir.LIMIT)}" in h and f"ALAC_RIR_TILE = {rir.TILE}u" in h
    assert f"ALAC_RIR_MAX_TAPS = {rir.MAX_TAPS}u" in h and rir.MAX_FRAMES == 1 << 20 and "ALAC_RIR_MAX_FRAMES = 1u << 20" in h
