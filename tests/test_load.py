"""alac.net_amd.load / load_batch: whole M4A files decoded on the GPU into one tensor, against the encoder's source PCM."""
import numpy as np
import pytest


def make_file(synth, n_packets, last, sample_size=16, stereo=True, seed=5, sample_rate=44100):
    from alac.net_amd.synth import m4a

    d = synth.packet_descs(n_packets, sample_size=sample_size, stereo=int(stereo), pred_order=8 if sample_size == 16 else 16)
    d["n"][-1] = last
    if sample_size == 24:
        d["ub"][::2] = 1
    b = synth.make_batch(d, synth.default_signal(seed), want_pcm=True)
    packets = [bytes(b["blob"][int(o):int(o) + int(s)]) for o, s in zip(b["offsets"], b["sizes"])]
    data = m4a.write_m4a(packets, [int(x) for x in d["n"]], sample_size=sample_size, channels=2 if stereo else 1,
                         sample_rate=sample_rate)
    ch = 2 if stereo else 1
    pcm = np.concatenate([b["pcm"][p, : int(d["n"][p]) * ch] for p in range(n_packets)]).reshape(-1, ch)   # [T, C]
    return data, pcm


def scaled(torch, pcm, sample_size, dtype):
    if dtype == torch.int32:
        return torch.from_numpy(pcm.astype(np.int32))
    return torch.from_numpy(pcm.astype(np.float32) * np.float32(2.0 ** -(sample_size - 1)))


@pytest.mark.gpu
@pytest.mark.parametrize("sample_size,stereo", [(16, True), (24, True), (16, False), (24, False)])
def test_load_equals_source_pcm(synth, sample_size, stereo):
    import torch

    import alac.net_amd as pkg

    data, pcm = make_file(synth, 9, 1234, sample_size, stereo)
    for dtype in (torch.float32, torch.int32):
        planar, rate = pkg.load(data, dtype=dtype)
        assert rate == 44100 and planar.is_cuda and planar.dtype == dtype
        assert planar.shape == (pcm.shape[1], 8 * 4096 + 1234)
        assert torch.equal(planar.cpu(), scaled(torch, pcm, sample_size, dtype).T.contiguous())
        inter, _ = pkg.load(data, dtype=dtype, layout="interleaved")
        assert inter.shape == (8 * 4096 + 1234, pcm.shape[1])
        assert torch.equal(inter.cpu(), scaled(torch, pcm, sample_size, dtype))
    with pytest.raises(ValueError):
        pkg.load(data, dtype=torch.float64)
    with pytest.raises(ValueError):
        pkg.load(data, layout="rows")


@pytest.mark.gpu
def test_load_names_the_packet_that_fails(synth):
    import alac.net_amd as pkg
    from alac.net_amd import container

    data, _ = make_file(synth, 5, 4096)
    t = container.packet_table(data)
    pos = data.index(bytes(t["blob"][int(t["offsets"][3]):int(t["offsets"][3]) + 16]))
    bad = bytearray(data)
    # packet 3 (a two-channel element): channel A's prediction type made non-zero -- the reference throws (AlacFile.cs:650)
    hassize = (bad[pos + 2] >> 4) & 1
    k = 23 + 32 * hassize + 16                       # header, sample count, mix shift / weight: then predictionType (4 bits)
    bad[pos + k // 8] |= 0x80 >> (k % 8)
    with pytest.raises(pkg.AlacGpuError, match="packet 3"):
        pkg.load(bytes(bad))


@pytest.mark.gpu
def test_load_batch_pads_with_zeros_and_reports_lengths(synth):
    import torch

    import alac.net_amd as pkg

    files = [make_file(synth, 3, 100, 16, True, seed=1), make_file(synth, 5, 4000, 24, True, seed=2),
             make_file(synth, 1, 17, 16, True, seed=3), make_file(synth, 4, 4096, 24, True, seed=4)]
    out, lengths, rate = pkg.load_batch([f[0] for f in files])
    T = [len(f[1]) for f in files]
    assert rate == 44100 and lengths.tolist() == T and out.shape == (4, 2, max(T)) and out.dtype == torch.float32
    o = out.cpu()
    for f, (data, pcm) in enumerate(files):
        ss = 16 if f in (0, 2) else 24
        assert torch.equal(o[f, :, :T[f]], scaled(torch, pcm, ss, torch.float32).T), f
        assert (o[f, :, T[f]:] == 0).all(), f
    out_i, lengths_i, _ = pkg.load_batch([f[0] for f in files], dtype=torch.int32, max_frames=4500)
    Tc = [min(t, 4500) for t in T]
    assert lengths_i.tolist() == Tc and out_i.shape == (4, 2, 4500)
    o = out_i.cpu()
    for f, (data, pcm) in enumerate(files):
        assert torch.equal(o[f, :, :Tc[f]], torch.from_numpy(pcm[:Tc[f]].astype(np.int32)).T), f
        assert (o[f, :, Tc[f]:] == 0).all(), f


@pytest.mark.gpu
def test_load_batch_refuses_mixed_channels_or_rates(synth):
    import alac.net_amd as pkg

    a = make_file(synth, 2, 10, 16, True)[0]
    with pytest.raises(ValueError, match="channels"):
        pkg.load_batch([a, make_file(synth, 2, 10, 16, False)[0]])
    with pytest.raises(ValueError, match="channels"):
        pkg.load_batch([a, make_file(synth, 2, 10, 16, True, sample_rate=48000)[0]])
