"""alac.net_amd/vad.py without a device: the decisions of `vad_host` and `vad_host_f32` against a table worked out by hand, the
two against one another on inputs that keep every energy outside the threshold's margin (asserted), all-voiced and all-unvoiced
rows; `select_host` against boolean indexing per row; and the argument checks of `EnergyVad`."""
import numpy as np
import pytest

from test_normalize_spec import noise, same_bits

#        t:  0   1   2   3   4   5   6   7
TRACK = [0, 10,  6, 10, 10,  0,  6, 10]
# scale 0: thr = 5, above it: 0 1 1 1 1 0 1 1.  scale 0.5 over all 8: thr = 5 + 0.5 * 52 / 8 = 8.25; over the first 6: 5 + 0.5 * 36 / 6
# = 8: above it 0 1 0 1 1 0 0 1.  With context 2 the counts num / den of that are, for v = 8,
#   1/3 2/4 3/5 3/5 2/5 3/5 2/4 1/3        and for v = 6        1/3 2/4 3/5 3/5 2/4 2/3
# 0.12: every num >= 1 passes.  0.6: 1.8, 2.4 and fl(5 * 0.6f) = 3 (a tie that rounds to even) are the bars.  1.0: num == den only.
TABLE = [   # (scale, context, proportion, v, mask)
    (0.0, 0, 0.6, 8, [0, 1, 1, 1, 1, 0, 1, 1]),
    (0.5, 0, 0.12, 8, [0, 1, 0, 1, 1, 0, 0, 1]),
    (0.5, 0, 0.6, 8, [0, 1, 0, 1, 1, 0, 0, 1]),
    (0.5, 0, 1.0, 8, [0, 1, 0, 1, 1, 0, 0, 1]),
    (0.5, 2, 0.12, 8, [1, 1, 1, 1, 1, 1, 1, 1]),
    (0.5, 2, 0.6, 8, [0, 0, 1, 1, 0, 1, 0, 0]),
    (0.5, 2, 1.0, 8, [0, 0, 0, 0, 0, 0, 0, 0]),
    (0.5, 2, 0.12, 6, [1, 1, 1, 1, 1, 1, 0, 0]),
    (0.5, 2, 0.6, 6, [0, 0, 1, 1, 0, 1, 0, 0]),
    (0.5, 2, 1.0, 6, [0, 0, 0, 0, 0, 0, 0, 0]),
    (0.0, 2, 0.8, 8, [0, 0, 1, 1, 1, 1, 0, 0]),         # 0 1 1 1 1 0 1 1: 2/3 3/4 4/5 4/5 4/5 4/5 3/4 2/3 against 2.4, 3.2, fl(5 * 0.8f) = 4
    (0.0, 2, 0.6, 3, [1, 1, 1]),                          # 0 1 1: den 3 everywhere, 2 >= 1.8
]


@pytest.mark.parametrize("scale,context,proportion,v,mask", TABLE)
def test_decisions_of_a_hand_made_track(scale, context, proportion, v, mask):
    from alac.net_amd.vad import EnergyVad, vad_host, vad_host_f32

    n = len(mask)
    x = np.full((2, 2, 3, n), np.nan, dtype=np.float32)     # line 1 of channel 0 is the energy; nothing else is looked at
    x[:, 0, 1, :] = TRACK[:n]
    x[1, 0, 1, v:] = np.nan                                  # row 1: not a frame at or behind v is looked at
    vad = EnergyVad(5.0, scale, context, proportion, line=1)
    for f in (vad_host, vad_host_f32):
        got = f(x, vad, [n if v == n else v, v])
        assert got.dtype == np.uint8 and got.shape == (2, n)
        assert got[0].tolist() == list(mask) and got[1].tolist() == list(mask), (f.__name__, got.tolist())
    assert vad_host(x[:, 0], vad, [v, v]).tolist() == [list(mask)] * 2       # [B, lines, n]


def clear_of_the_threshold(shape, seed, vad, lengths):
    """Energies around 8 +- 6 of which none is within 1e-3 of the specification's threshold"""
    from alac.net_amd.vad import vad_host

    x = (8.0 + 6.0 * noise(shape, seed).astype(np.float64)).astype(np.float32)
    _, dist, _ = vad_host(x, vad, lengths, margin=True)
    E = x[:, 0, vad.line, :] if x.ndim == 4 else x[:, vad.line, :]
    E[dist < 1e-3] += np.float32(0.5)           # (a view: x changes; the mean moves by far less than the 0.5)
    return x


def test_the_twin_decides_as_the_specification_outside_the_margin():
    from alac.net_amd.vad import EnergyVad, vad_host, vad_host_f32

    checked = 0
    for shape, lengths in (((4, 1, 13, 200), [200, 77, 0, -1]), ((3, 2, 30, 300), [300, 299, 5]), ((2, 5, 1000), None)):
        for vad in (EnergyVad(), EnergyVad.voxceleb(), EnergyVad(5.5, 0.5, 2, 0.12, line=3), EnergyVad(6.0, 0.0, 64, 1.0),
                    EnergyVad(-2.0, 1.0, 1, 0.0)):
            x = clear_of_the_threshold(shape, 3, vad, lengths)
            mask, dist, dthr = vad_host(x, vad, lengths, margin=True)
            assert (dist > dthr[:, None]).all(), "an energy within the margin of the threshold: the input excuses nothing"
            assert (dthr < 1e-3).all()
            got = vad_host_f32(x, vad, lengths)
            assert np.array_equal(got, mask), (shape, vad)
            v = np.clip(np.asarray(lengths if lengths is not None else [shape[-1]] * shape[0]), 0, shape[-1])
            for b, k in enumerate(v):
                assert (mask[b, k:] == 0).all() and np.isinf(dist[b, k:]).all()
            checked += int(mask.sum())
    assert checked > 1000


def test_all_voiced_all_unvoiced_and_nan():
    from alac.net_amd.vad import EnergyVad, vad_host, vad_host_f32

    x = noise((3, 1, 2, 50), 1)
    x[0, 0, 0] += 20.0
    x[1, 0, 0] -= 20.0
    x[2, 0, 0, 7] = np.nan
    for f in (vad_host, vad_host_f32):
        got = f(x, EnergyVad(5.0, 0.0, 2, 0.6), [50, 50, 50])
        assert (got[0] == 1).all() and (got[1] == 0).all() and (got[2] == 0).all()
        # the mean of a row with a NaN is NaN: nothing is above it; with a proportion of 0 every frame still passes 0 >= 0
        assert (f(x, EnergyVad(-50.0, 0.5, 0, 0.6), [50, 50, 50])[2] == 0).all()
        assert (f(x, EnergyVad(-50.0, 0.0, 0, 0.6), [50, 50, 50])[2] == (np.arange(50) != 7)).all()     # scale 0: no mean
        assert (f(x, EnergyVad(5.0, 0.5, 3, 0.0), [50, 20, 50])[1] == (np.arange(50) < 20)).all()
    for bad in ((x.astype(np.float64), EnergyVad()), (x, "vad"), (x, EnergyVad(line=2)), (x[0, 0], EnergyVad()), (x, EnergyVad(), [1, 2])):
        with pytest.raises(ValueError):
            vad_host(*bad)
        with pytest.raises(ValueError):
            vad_host_f32(*bad)


def test_select_host_is_boolean_indexing_per_row():
    from alac.net_amd.vad import select_host

    rng = np.random.default_rng(5)
    n = 37
    x = noise((5, 2, 3, n), 2)
    mask = (rng.uniform(size=(5, n)) < 0.5).astype(np.uint8)
    mask[1] = 1
    mask[2] = 0
    lengths = [n, 20, n, -1, n + 9]
    y, new = select_host(x, mask, lengths)
    assert y.shape == x.shape and y.dtype == x.dtype and new.dtype == np.int64
    for b, given in enumerate(lengths):
        v = min(max(given, 0), n)
        keep = mask[b].astype(bool) & (np.arange(n) < v)
        k = int(keep.sum())
        assert same_bits(y[b][..., :k], x[b][..., keep]), b
        assert (y[b][..., k:] == 0).all(), b
        assert new[b] == (given if given < 0 else k), b
    assert new.tolist() == [int(mask[0].sum()), 20, 0, -1, int(mask[4].sum())]
    # without lengths, bool masks, [B, n] data, an integer dtype: bits move
    z, new = select_host(x[:, 0, 0].view(np.int32), mask.astype(bool))
    assert z.dtype == np.int32 and new.tolist() == mask.sum(axis=1).tolist()
    assert np.array_equal(z[0, :new[0]], x[0, 0, 0].view(np.int32)[mask[0].astype(bool)])
    for bad in ((x, mask[:, :-1]), (x, mask[:4]), (x[0, 0, 0], mask[0]), (x, mask, [1, 2])):
        with pytest.raises(ValueError):
            select_host(*bad)


def test_energy_vad_arguments_and_immutability():
    import alac.net_amd as pkg
    from alac.net_amd.vad import EnergyVad

    d = EnergyVad()
    assert (d.energy_threshold, d.energy_mean_scale, d.frames_context, d.proportion_threshold, d.line) == (5.0, 0.5, 0, 0.6, 0)
    vc = EnergyVad.voxceleb()
    assert (vc.energy_threshold, vc.energy_mean_scale, vc.frames_context, vc.proportion_threshold, vc.line) == (5.5, 0.5, 2, 0.12, 0)
    assert pkg.EnergyVad is EnergyVad and vc == EnergyVad(5.5, 0.5, 2, 0.12) and vc != d and hash(vc) == hash(EnergyVad(5.5, 0.5, 2, 0.12))
    for kw in (dict(energy_threshold=float("nan")), dict(energy_threshold=float("inf")), dict(energy_threshold=1e39),
               dict(energy_threshold="5"), dict(energy_mean_scale=-0.1), dict(energy_mean_scale=float("inf")),
               dict(frames_context=-1), dict(frames_context=65), dict(frames_context=1.0), dict(frames_context=True),
               dict(proportion_threshold=-0.01), dict(proportion_threshold=1.01), dict(proportion_threshold=float("nan")),
               dict(line=-1), dict(line=0.0)):
        with pytest.raises(ValueError):
            EnergyVad(**kw)
    assert EnergyVad(frames_context=64, proportion_threshold=1.0, energy_mean_scale=0.0, energy_threshold=-3.0).frames_context == 64
    with pytest.raises(AttributeError):
        d.line = 1
    with pytest.raises(AttributeError):
        del d.energy_threshold
    for name in ("vad_energy", "select_frames", "vad_host", "vad_host_f32", "select_host", "sliding_host", "sliding_host_f32"):
        assert callable(getattr(pkg, name))
