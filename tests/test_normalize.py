"""alacgpu_normalize_meanvar_device and alacgpu_normalize_top_device on the GPU against their specification in numpy
(alac.net_amd/normalize.py), then `normalize` and Corpus.crops(normalize=).

MeanVar: |got - y| <= dY for every element, y and dY from normalize_host(..., bound=True) (the chain derived in normalize.py);
where y is NaN (a constant line without eps: 0 / 0) got is NaN.  dY holds for any order of the sums and is 50 to 1000 times
what a correct evaluation costs, so there is the second yardstick of tests/test_features.py's check_power, with its factor:
r = max |. - y| / dY over the elements whose dY is finite and positive, and r_gpu <= 4 r_twin with the twin
normalize_host_f32, the kernel's arithmetic in numpy -- on full-scale noise and on 0.9 + 1e-3 * noise, where
tests/test_normalize_spec.py shows a one-pass variance to miss the criterion by a factor of a thousand.  Elements at or
behind v are exactly 0.

TopDb: every operation is exactly rounded, so got equals normalize_host_f32 bit for bit, zeros comparing equal.

Every call reads source lines that carry NaN behind line_len and writes into an output prefilled with NaN between guards of
0x5A bytes: what lies behind line_len in the output and the guards are intact after every call.  Shapes are chosen by code
path: both sides of every threshold of csrc/alac_normalize.h."""
import numpy as np
import pytest

from test_features import header_constant
from test_normalize_spec import dc, noise, same_bits

pytestmark = pytest.mark.gpu

GUARD = 64
SLACK = 5


def constant(name):
    return header_constant(name, "alac_normalize.h")


@pytest.fixture(scope="module")
def gpu():
    import torch

    import alac.net_amd as pkg

    with pkg.AlacGpuContext([(4096, 16, 40, 10, 14, 2)], device=0) as ctx:
        yield torch, ctx


def run(gpu, x, how, valid=None, slack=SLACK, in_place=False):
    """One call of the context method of `how` over x [rows, lines_per_row, n] (numpy float32): the source with `slack` NaNs
    behind every line, the output of the same layout prefilled with NaN between two guards (in_place: the source lives
    there).  Returns out [rows, lines_per_row, n] as numpy after checking the guards and what lies behind the lines."""
    from alac.net_amd.normalize import MeanVar

    torch, ctx = gpu
    dev = torch.device("cuda", 0)
    rows, lpr, n = x.shape
    S = n + slack
    src = np.full((rows, lpr, S), np.nan, dtype=np.float32)
    src[:, :, :n] = x
    total = rows * lpr * S
    raw = torch.full(((total + 2 * GUARD) * 4,), 0x5A, dtype=torch.uint8, device=dev).view(torch.float32)
    out = raw[GUARD:GUARD + total]
    d_src = torch.from_numpy(src).to(dev)
    if in_place:
        out.copy_(d_src.flatten())
        d_src = out
    else:
        out.fill_(float("nan"))
    stream = torch.cuda.current_stream().cuda_stream
    if isinstance(how, MeanVar):
        d_valid = None if valid is None else torch.tensor(list(valid), dtype=torch.int64, device=dev)
        ctx.normalize_meanvar_device(d_src, out, rows, lpr, S, n, d_valid, how.centre, how.scale, how.eps, stream=stream)
    else:
        assert not how.per_channel
        ctx.normalize_top_device(d_src, out, rows, lpr, S, n, how.top, how.scale, how.offset, how.relative, stream=stream)
    torch.cuda.synchronize()
    assert bool((torch.cat([raw[:GUARD], raw[GUARD + total:]]).view(torch.uint8) == 0x5A).all()), "a guard was written"
    got = out.cpu().numpy().reshape(rows, lpr, S)
    assert np.isnan(got[:, :, n:]).all(), "an element behind line_len was written"
    if not in_place:
        back = d_src.cpu().numpy()
        assert np.array_equal(back[:, :, :n], x, equal_nan=True) and np.isnan(back[:, :, n:]).all(), "the source was written"
    return got[:, :, :n].copy()


def check_meanvar(got, x, how, valid, tag, twin=True):
    """|got - y| <= dY, NaN where y is NaN, the same infinity where y is one, zeros behind v; twin: r_gpu <= 4 r_twin"""
    from alac.net_amd.normalize import normalize_host, normalize_host_f32

    y, dY = normalize_host(x, how, valid, bound=True)
    n = x.shape[-1]
    v = np.clip(np.asarray(valid if valid is not None else [n] * x.shape[0]), 0, n)
    for b, k in enumerate(v):
        assert (got[b, :, k:] == 0).all(), (tag, "not zero behind v", b)
    nan = np.isnan(y)
    assert np.array_equal(np.isnan(got), nan), (tag, "NaN where the specification has none, or none where it has")
    inf = np.isinf(y)                   # (a line of one element with centre off and no eps: x / 0)
    assert np.array_equal(got[inf].astype(np.float64), y[inf]), (tag, "an infinity of the specification is not one of the kernel")
    with np.errstate(all="ignore"):
        err = np.where(nan | inf, 0.0, np.abs(got.astype(np.float64) - y))
        assert (nan | inf | (err <= dY)).all(), (tag, int(np.argmax(np.where(nan | inf, -np.inf, err - dY))), float(err.max()))
        live = ~nan & ~inf & np.isfinite(dY) & (dY > 0)
        if twin and live.any():
            t = normalize_host_f32(x, how, valid)
            r_gpu = float(np.max(err[live] / dY[live]))
            r_ref = float(np.max(np.abs(t.astype(np.float64) - y)[live] / dY[live]))
            print(f"{tag}: r_gpu {r_gpu:.5f}, r_twin {r_ref:.5f}, equal bits {same_bits(got, t)}")
            assert r_gpu <= 4 * r_ref, (tag, r_gpu, r_ref)


def line_lengths():
    wave, lds = constant("ALAC_NORM_WAVE_MAX"), constant("ALAC_NORM_LDS_MAX")
    return sorted({1, 2, 63, 64, 65, 255, 256, 257, wave - 1, wave, wave + 1, lds - 1, lds, lds + 1})


def valid_for(n, rows, turn):
    """`rows` lengths out of -1, 0, 1, n, n + 5 and values in between, another selection every turn"""
    pool = [-1, 0, 1, n, n + 5, n // 2, max(n - 1, 0), (2 * n) // 3, 2]
    return [pool[(turn + 4 * r) % len(pool)] for r in range(rows)]


@pytest.mark.parametrize("n", line_lengths())
def test_meanvar_grid(gpu, n):
    from alac.net_amd.normalize import MeanVar

    turn = 7 * n
    for lpr in (1, 3, 80):
        for rows in (1, 3):
            x = noise((rows, lpr, n), 100 + turn)
            how = MeanVar() if turn % 3 else MeanVar(eps=1e-5)
            tag = f"n {n} lines {lpr} rows {rows} {how}"
            check_meanvar(run(gpu, x, how), x, how, None, tag + " whole")
            valid = valid_for(n, rows, turn)
            check_meanvar(run(gpu, x, how, valid), x, how, valid, tag + f" valid {valid}")
            turn += 1


def mapping_lengths():
    """a line length in each of the three mappings"""
    return [201, constant("ALAC_NORM_WAVE_MAX") + 44, constant("ALAC_NORM_LDS_MAX") + 100]


@pytest.mark.parametrize("n", mapping_lengths())
def test_meanvar_on_noise_and_on_a_dc_offset_in_every_mapping(gpu, n):
    """Every length of the pool in one call, centre and scale alone, full-scale noise and 0.9 + 1e-3 * noise"""
    from alac.net_amd.normalize import MeanVar

    valid = [-1, 0, 1, 2, n // 2, n - 1, n, n + 5]
    for make, name in ((noise, "noise"), (dc, "dc")):
        x = make((len(valid), 3, n), 7)
        for how in (MeanVar(), MeanVar(eps=1e-5), MeanVar(scale=False), MeanVar(centre=False)):
            check_meanvar(run(gpu, x, how, valid), x, how, valid, f"{name} n {n} {how}")
            check_meanvar(run(gpu, x, how), x, how, None, f"{name} n {n} {how} whole")


def top_cases():
    """(lines_per_row, line_len) of rows of 1, 255, 256, 257 elements and of both sides of every boundary between parts up to
    three parts, as one line and as several"""
    part = constant("ALAC_TOP_PART")
    assert constant("ALAC_TOP_MAX_PARTS") >= 3
    sizes = sorted({1, 255, 256, 257, part - 1, part, part + 1, 2 * part - 1, 2 * part, 2 * part + 1})
    shapes = [(1, s) for s in sizes]
    for s in sizes:
        for lines in (3, 5, 16):
            if s % lines == 0 and s > lines:
                shapes.append((lines, s // lines))
                break
    return part, shapes


def test_top_grid(gpu):
    from alac.net_amd.normalize import TopDb, normalize_host_f32

    part, shapes = top_cases()
    calls = 0
    for lpr, n in shapes:
        size = lpr * n
        # three rows: the maximum at the first element, at the last, and at the first element of the last part
        x = np.random.default_rng(size).uniform(-10.0, 2.0, (3, lpr * n)).astype(np.float32)
        x[0, 0] = x[1, size - 1] = x[2, (size - 1) // part * part] = np.float32(2.5)
        x = x.reshape(3, lpr, n)
        for relative in (False, True):
            for top in (0.0, 8.0):
                for scale, offset in ((1.0, 0.0), (0.25, 1.0), (10.0, 0.0)):
                    how = TopDb(top, scale, offset, relative)
                    got = run(gpu, x, how)
                    want = normalize_host_f32(x, how)
                    assert same_bits(got, want), (lpr, n, how, int(np.argmax(got != want)))
                    calls += 1
    print(f"{calls} calls over {len(shapes)} shapes, parts of {part}")


def property_cases():
    from alac.net_amd.normalize import MeanVar, TopDb

    wave, lds, part = constant("ALAC_NORM_WAVE_MAX"), constant("ALAC_NORM_LDS_MAX"), constant("ALAC_TOP_PART")
    cases = [(MeanVar(), (3, 4, n), [n - 7, -1, n // 2]) for n in (wave - 55, wave + 300, lds + 100)]
    cases += [(MeanVar(centre=False, eps=1e-5), (3, 2, wave + 300), None)]
    cases += [(how, shape, None) for how in (TopDb.whisper(), TopDb.decibels(80.0, relative=True))
              for shape in ((3, 1, 200), (3, 7, (2 * part + 50) // 7))]
    return cases


def test_in_place_batches_and_strides_change_nothing(gpu):
    for k, (how, shape, valid) in enumerate(property_cases()):
        x = np.random.default_rng(k).uniform(-3.0, 1.0, shape).astype(np.float32)
        ref = run(gpu, x, how, valid)
        assert same_bits(run(gpu, x, how, valid, in_place=True), ref), (how, shape, "in place")
        assert same_bits(run(gpu, x, how, valid, slack=0), ref), (how, shape, "line_stride == line_len")
        assert same_bits(run(gpu, x, how, valid, slack=0, in_place=True), ref), (how, shape, "in place, line_stride == line_len")
        for r in range(shape[0]):
            alone = run(gpu, x[r:r + 1], how, None if valid is None else valid[r:r + 1])
            assert same_bits(alone[0], ref[r]), (how, shape, "row alone", r)


def test_what_is_not_finite_stays_where_it_is(gpu):
    from alac.net_amd.normalize import MeanVar, TopDb

    for k, (how, shape, valid) in enumerate(property_cases()):
        x = np.random.default_rng(50 + k).uniform(-3.0, 1.0, shape).astype(np.float32)
        ref = run(gpu, x, how, valid)
        n = shape[-1]
        for bad in (np.nan, np.inf):
            z = x.copy()
            z[0, shape[1] - 1, n // 3] = bad               # row 0, its last line; inside v (valid[0] = n - 7)
            got = run(gpu, z, how, valid)
            assert same_bits(got[1:], ref[1:]), (how, shape, bad, "another row changed")
            if isinstance(how, MeanVar):
                assert same_bits(got[0, :-1], ref[0, :-1]), (how, shape, bad, "another line changed")
                v = n if valid is None else valid[0]
                assert np.isnan(got[0, -1, :v]).all() and (got[0, -1, v:] == 0).all(), (how, shape, bad)
            elif np.isnan(bad):
                assert np.isnan(got[0]).all(), (how, shape, "the row with the NaN is NaN throughout")
            else:                                          # mx = +inf: c = +inf, z = +inf; relative: inf - inf
                want = np.nan if how.relative else np.inf
                assert same_bits(got[0], np.full_like(got[0], want)), (how, shape, "mx = +inf")
        if isinstance(how, MeanVar) and valid is not None:
            z = x.copy()
            z[0, 0, valid[0]] = np.nan                     # at v
            z[0, 1, n - 1] = np.inf                        # behind v
            z[1] = np.nan                                  # valid[1] = -1: nothing of the row is read
            assert same_bits(run(gpu, z, how, valid), ref), (how, shape, "a NaN at or behind v changed something")
            assert same_bits(run(gpu, z, how, valid, in_place=True), ref), (how, shape, "... in place")


def test_the_public_call(gpu):
    from alac.net_amd.normalize import MeanVar, TopDb, normalize, normalize_host, normalize_host_f32

    torch, _ = gpu
    x = np.random.default_rng(9).uniform(-10.0, 2.0, (3, 2, 80, 50)).astype(np.float32)
    d = torch.from_numpy(x).cuda()
    lengths = [50, 23, -1]
    # MeanVar with lengths: a sequence, a device tensor, in place
    y, dY = normalize_host(x, MeanVar(), lengths, bound=True)
    got = normalize(d, MeanVar(), lengths)
    assert got.shape == d.shape and got.is_contiguous() and got.data_ptr() != d.data_ptr() and torch.equal(d.cpu(), torch.from_numpy(x))
    g = got.cpu().numpy()
    assert (np.abs(g.astype(np.float64) - y) <= dY).all() and (g[1, ..., 23:] == 0).all() and (g[2] == 0).all()
    assert same_bits(g, normalize_host_f32(x, MeanVar(), lengths))
    assert torch.equal(normalize(d, MeanVar(), torch.tensor(lengths, device="cuda")), got)
    assert torch.equal(normalize(d, MeanVar(), torch.tensor(lengths, dtype=torch.int32)), got)
    e = d.clone()
    assert normalize(e, MeanVar(), lengths, out=e) is e and torch.equal(e, got)
    # TopDb: per crop and per channel; lengths are not TopDb's
    for how in (TopDb.whisper(), TopDb(8.0, 0.25, 1.0, per_channel=True), TopDb.decibels(80.0, relative=True)):
        assert same_bits(normalize(d, how, lengths).cpu().numpy(), normalize_host_f32(x, how)), how
    assert not same_bits(normalize_host_f32(x, TopDb.whisper()), normalize_host_f32(x, TopDb(8.0, 0.25, 1.0, per_channel=True)))
    # the slice [..., :49]: Whisper's dropped last frame; the 50th column is neither read nor written
    z = x.copy()
    z[..., 49] = np.nan
    for how, lens in ((TopDb.whisper(), None), (MeanVar(), [49, 23, -1]), (TopDb(per_channel=True), None)):
        want = normalize_host_f32(np.ascontiguousarray(x[..., :49]), how, lens)
        dz = torch.from_numpy(z).cuda()
        got = normalize(dz[..., :-1], how, lens)                     # out of place: a new tensor of the slice's layout
        assert got.shape == (3, 2, 80, 49) and same_bits(got.cpu().numpy(), want), how
        assert torch.equal(dz.cpu().view(torch.int32), torch.from_numpy(z).view(torch.int32)), how
        assert normalize(dz[..., :-1], how, lens, out=dz[..., :-1]).data_ptr() == dz.data_ptr()
        back = dz.cpu().numpy()
        assert same_bits(back[..., :49], want) and np.isnan(back[..., 49]).all(), how
    # [B, n], a waveform without a channel dimension, and an empty batch
    w = noise((4, 1000), 3)
    assert same_bits(normalize(torch.from_numpy(w).cuda(), MeanVar(), [1000, 1, 500, 0]).cpu().numpy(),
                     normalize_host_f32(w, MeanVar(), [1000, 1, 500, 0]))
    assert normalize(d[:0], MeanVar()).shape == (0, 2, 80, 50)
    # ValueError before any device work
    for args in ((d.cpu(), MeanVar()), (d.double(), MeanVar()), (d, "whisper"), (d[..., ::2], MeanVar()), (d[:, :, :40], TopDb()),
                 (d.transpose(2, 3), MeanVar()), (d[0, 0, 0], MeanVar()), (d[:, 0, 0], TopDb(per_channel=True)),
                 (d, MeanVar(), [1, 2]), (d, MeanVar(), [1.0, 2.0, 3.0]), (d, MeanVar(), torch.ones(3, device="cuda"))):
        with pytest.raises(ValueError):
            normalize(*args)
    for out in (d[..., :49], d.double(), d.cpu(), torch.empty(3, 2, 80, 51, device="cuda")[..., :50]):
        with pytest.raises(ValueError):
            normalize(d, TopDb(), out=out)


L = 3000


@pytest.fixture(scope="module")
def corpus(synth):
    import alac.net_amd as pkg
    from test_load_window import make_file

    files = [make_file(synth, n, last, ss, True, seed=30 + i)[0] for i, (n, last, ss) in enumerate([(3, 100, 16), (2, 4000, 24), (4, 1234, 16)])]
    with pkg.Corpus(files) as c:
        yield c


def device_crops(torch, corpus, totals):
    """Crops as device tensors: a start, a middle, one that runs off its file's end, and the last outside the corpus"""
    cf = [0, 1, 2, 2, corpus.num_files]
    co = [0, int(totals[1]) // 3, max(int(totals[2]) - L // 2, 0), 17, 0]
    return torch.tensor(cf, device="cuda"), torch.tensor(co, device="cuda")


def test_corpus_features_are_normalised_as_normalize_does(gpu, corpus):
    import alac.net_amd as pkg

    torch, _ = gpu
    spec = pkg.LogMel(44100, 400, 160, 80, log="log10")
    d_f, d_o = device_crops(torch, corpus, corpus.num_frames)
    feats, flen = corpus.crops(d_f, d_o, L, features=spec, check=False)
    feats = feats.clone()
    assert flen.tolist()[-1] == -1 and flen.tolist()[2] == (L // 2) // 160 + 1
    for how in (pkg.TopDb.whisper(), pkg.TopDb(per_channel=True), pkg.TopDb.decibels(80.0, relative=True), pkg.MeanVar(),
                pkg.MeanVar(eps=1e-5, scale=False)):
        want = pkg.normalize(feats, how, flen)
        got, glen = corpus.crops(d_f, d_o, L, features=spec, check=False, normalize=how)
        assert got.shape == feats.shape and torch.equal(glen, flen), how
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), how
        if isinstance(how, pkg.MeanVar):
            assert (got[-1] == 0).all() and (got[2, ..., int(flen[2]):] == 0).all() and torch.isfinite(got).all(), how
        st, mask = corpus.last_status()
        assert st.numel() > 0 and mask.shape == st.shape          # last_status() is the crops' own
        out = torch.empty_like(feats)
        assert corpus.crops(d_f, d_o, L, features=spec, check=False, normalize=how, out=out)[0] is out and torch.equal(out, got)
    # check=True still names the crop outside the corpus
    with pytest.raises(ValueError):
        corpus.crops(d_f, d_o, L, features=spec, normalize=pkg.MeanVar())
    res = corpus.random_crops(6, L, generator=torch.Generator().manual_seed(3), features=spec, normalize=pkg.TopDb.whisper())
    want = corpus.crops(res[2], res[3], L, features=spec)[0]
    assert torch.equal(res[0], pkg.normalize(want, pkg.TopDb.whisper()))


def test_corpus_crops_have_zero_mean_and_unit_variance(gpu, corpus):
    import alac.net_amd as pkg

    torch, _ = gpu
    how = pkg.MeanVar()
    for tag, kw, totals in (("native", {}, corpus.num_frames),
                            ("16 kHz mono", dict(sample_rate=16000, mono=True), corpus.resampled_frames(16000))):
        d_f, d_o = device_crops(torch, corpus, totals)
        pcm, lengths = corpus.crops(d_f, d_o, L, check=False, **kw)
        pcm = pcm.clone()
        got, glen = corpus.crops(d_f, d_o, L, check=False, normalize=how, **kw)
        assert torch.equal(glen, lengths) and got.shape == pcm.shape and got.dtype == torch.float32, tag
        assert torch.equal(got.view(torch.int32), pkg.normalize(pcm, how, lengths).view(torch.int32)), tag
        _, dY = pkg.normalize_host(pcm.cpu().numpy(), how, lengths.tolist(), bound=True)
        g = got.cpu().numpy().astype(np.float64)
        lens = lengths.tolist()
        assert lens[-1] == -1 and (g[-1] == 0).all(), tag
        assert 0 < lens[2] < L, tag
        for b, v in enumerate(lens[:-1]):
            assert v > 1 and (g[b, :, v:] == 0).all(), (tag, b)
            for c in range(g.shape[1]):
                bound = float(dY[b, c, :v].max())
                m, ms = float(g[b, c, :v].mean()), float((g[b, c, :v] ** 2).mean())
                print(f"{tag} crop {b} channel {c}: v {v}, mean {m:.3e}, mean square - 1 {ms - 1:.3e}, max dY {bound:.3e}")
                assert abs(m) <= bound and abs(ms - 1.0) <= bound, (tag, b, c)
    res = corpus.random_crops(5, L, generator=torch.Generator().manual_seed(4), normalize=how)
    assert res[0].shape == (5, corpus.channels, L) and torch.equal(res[0], pkg.normalize(corpus.crops(res[2], res[3], L)[0], how, res[1]))


def test_corpus_refuses_what_cannot_be_normalised(gpu, corpus):
    import alac.net_amd as pkg

    torch, _ = gpu
    before = corpus.last_status()[0].clone()
    with pytest.raises(ValueError):
        corpus.crops([0], [0], L, normalize=pkg.TopDb.whisper())                       # a TopDb without features
    with pytest.raises(ValueError):
        corpus.crops([0], [0], L, dtype=torch.int32, normalize=pkg.MeanVar())          # a MeanVar with int32 crops
    with pytest.raises(ValueError):
        corpus.crops([0], [0], L, normalize="meanvar")
    with pytest.raises(ValueError):
        corpus.random_crops(2, L, normalize=pkg.TopDb())
    assert torch.equal(corpus.last_status()[0], before)                                # nothing ran
