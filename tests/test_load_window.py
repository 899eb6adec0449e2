"""load(frame_offset=, num_frames=) and load_batch(frame_offsets=): windows of M4A files decoded on the GPU, against the
encoder's source PCM sliced; only the packets that overlap a window are decoded."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def make_file(synth, n_packets, last, sample_size=16, stereo=True, seed=5):
    """An M4A file of n_packets - 1 packets of 4096 frames and one of `last`, and its source PCM [T, C]"""
    from alac.net_amd.synth import m4a

    d = synth.packet_descs(n_packets, sample_size=sample_size, stereo=int(stereo), pred_order=8 if sample_size == 16 else 16)
    d["n"][-1] = last
    if sample_size == 24:
        d["ub"][::2] = 1
    b = synth.make_batch(d, synth.default_signal(seed), want_pcm=True)
    packets = [bytes(b["blob"][int(o):int(o) + int(s)]) for o, s in zip(b["offsets"], b["sizes"])]
    data = m4a.write_m4a(packets, [int(x) for x in d["n"]], sample_size=sample_size, channels=2 if stereo else 1,
                         sample_rate=44100)
    ch = 2 if stereo else 1
    pcm = np.concatenate([b["pcm"][p, : int(d["n"][p]) * ch] for p in range(n_packets)]).reshape(-1, ch)
    return data, pcm


def scaled(torch, pcm, sample_size, dtype):
    if dtype == torch.int32:
        return torch.from_numpy(pcm.astype(np.int32))
    return torch.from_numpy(pcm.astype(np.float32) * np.float32(2.0 ** -(sample_size - 1)))


def corrupt(data, packet):
    """The file with channel A's prediction type of `packet` (a two-channel element) made non-zero: the reference throws
    (AlacFile.cs:650), status 6"""
    from alac.net_amd import container

    t = container.packet_table(data)
    o = int(t["offsets"][packet])
    pos = data.index(bytes(t["blob"][o:o + 16]))
    bad = bytearray(data)
    hassize = (bad[pos + 2] >> 4) & 1
    k = 23 + 32 * hassize + 16
    bad[pos + k // 8] |= 0x80 >> (k % 8)
    return bytes(bad)


@pytest.mark.parametrize("sample_size,stereo", [(16, True), (24, True), (16, False), (24, False)])
def test_load_windows_equal_the_source_slice(synth, sample_size, stereo):
    import torch

    import alac.net_amd as pkg

    data, pcm = make_file(synth, 9, 1234, sample_size, stereo)
    T = 8 * 4096 + 1234
    assert pkg.info(data)["num_frames"] == T == len(pcm)
    windows = [(0, None), (0, 1), (0, 5000), (2500, 3000), (2500, None), (3 * 4096, 4096), (3 * 4096, 1), (3 * 4096 - 1, 2),
               (8 * 4096 + 100, None), (8 * 4096 + 100, 50), (T - 1, None), (T - 1, 10 ** 9), (T, None), (T, 5), (17, 0)]
    for off, num in windows:
        n = T - off if num is None else min(num, T - off)
        for dtype in (torch.float32, torch.int32):
            want = scaled(torch, pcm[off:off + n], sample_size, dtype)
            planar, rate = pkg.load(data, dtype=dtype, frame_offset=off, num_frames=num)
            assert rate == 44100 and planar.dtype == dtype and planar.shape == (pcm.shape[1], n), (off, num)
            assert torch.equal(planar.cpu(), want.T.contiguous()), (off, num, dtype)
            inter, _ = pkg.load(data, dtype=dtype, layout="interleaved", frame_offset=off, num_frames=num)
            assert inter.shape == (n, pcm.shape[1]), (off, num)
            assert torch.equal(inter.cpu(), want), (off, num, dtype)


def test_load_batch_windows_padding_and_lengths(synth):
    import torch

    import alac.net_amd as pkg

    files = [make_file(synth, 3, 100, 16, True, seed=1), make_file(synth, 5, 4000, 24, True, seed=2),
             make_file(synth, 1, 17, 16, True, seed=3), make_file(synth, 4, 4096, 24, True, seed=4)]
    T = [len(f[1]) for f in files]
    sizes = [16, 24, 16, 24]
    for offsets, max_frames in (([5000, 4096 * 2 + 1, 3, 0], None), ([8292, 1, 17, 12000], 3000), (7, 2000), ([0, 0, 0, 0], 100),
                                ([T[0], T[1], T[2], T[3]], None)):
        offs = [offsets] * 4 if np.ndim(offsets) == 0 else offsets
        want_len = [min(t - o, max_frames if max_frames is not None else t) for t, o in zip(T, offs)]
        for dtype in (torch.float32, torch.int32):
            out, lengths, rate = pkg.load_batch([f[0] for f in files], dtype=dtype, max_frames=max_frames, frame_offsets=offsets)
            assert rate == 44100 and lengths.tolist() == want_len and out.shape == (4, 2, max(want_len)) and out.dtype == dtype
            o = out.cpu()
            for f, (data, pcm) in enumerate(files):
                L = want_len[f]
                want = scaled(torch, pcm[offs[f]:offs[f] + L], sizes[f], dtype).T
                assert torch.equal(o[f, :, :L], want), (offsets, max_frames, f)
                assert (o[f, :, L:] == 0).all(), (offsets, max_frames, f)
    # the defaults are the whole files, as before
    out, lengths, _ = pkg.load_batch([f[0] for f in files], frame_offsets=0)
    assert lengths.tolist() == T


def test_a_corrupt_packet_outside_the_window_is_never_decoded(synth):
    import torch

    import alac.net_amd as pkg

    data, pcm = make_file(synth, 6, 2000)
    bad = corrupt(data, 2)
    with pytest.raises(pkg.AlacGpuError, match="packet 2"):
        pkg.load(bad)
    # windows that leave packet 2 (frames 8192 .. 12288) out load, and equal the source
    for off, num in ((0, 8192), (12288, None), (100, 8000), (12289, 5)):
        got, _ = pkg.load(bad, dtype=torch.int32, frame_offset=off, num_frames=num)
        n = got.shape[1]
        assert torch.equal(got.cpu(), torch.from_numpy(pcm[off:off + n].astype(np.int32)).T.contiguous()), (off, num)
    # one frame of it is enough to decode it, and the error names it by its index in the file
    for off, num in ((8191, 2), (12287, 10), (9000, 1)):
        with pytest.raises(pkg.AlacGpuError, match="packet 2 "):
            pkg.load(bad, frame_offset=off, num_frames=num)
    good, _ = make_file(synth, 4, 4096, seed=9)
    out, lengths, _ = pkg.load_batch([good, bad], frame_offsets=[0, 12288], max_frames=4096)
    assert lengths.tolist() == [4096, 4096]
    with pytest.raises(pkg.AlacGpuError, match="source 1, packet 2 "):
        pkg.load_batch([good, bad], frame_offsets=[0, 12000], max_frames=4096)


def test_a_packet_longer_than_16384_frames_in_its_stts_duration(synth):
    # packet 1 decodes 4096 frames but its stts duration is 20000: the whole file holds its frames, then zeros up to 20000.
    # A window starting more than 16384 frames into it gives those zeros too (no error), and the frames behind them.
    import torch

    import alac.net_amd as pkg
    from alac.net_amd.synth import m4a

    d = synth.packet_descs(4, stereo=1)
    b = synth.make_batch(d, synth.default_signal(12))
    packets = [bytes(b["blob"][int(o):int(o) + int(s)]) for o, s in zip(b["offsets"], b["sizes"])]
    data = m4a.write_m4a(packets, [4096, 20000, 4096, 4096], sample_size=16, channels=2, sample_rate=44100)
    T = 4096 + 20000 + 2 * 4096
    whole, _ = pkg.load(data, dtype=torch.int32)
    assert whole.shape == (2, T)
    w = whole.cpu()
    assert (w[:, 8192:24096] == 0).all() and (w[:, 4096:8192] != 0).any()
    for off, num in ((4096 + 17000, 100), (4096 + 17000, 8000), (4096 + 16000, 1000), (4096 + 16384, 3616), (4096 + 19999, 2),
                     (4096 + 16385, None), (4000, 20200)):
        got, _ = pkg.load(data, dtype=torch.int32, frame_offset=off, num_frames=num)
        n = got.shape[1]
        assert n == (T - off if num is None else min(num, T - off))
        assert torch.equal(got.cpu(), w[:, off:off + n]), (off, num)
    offs = [4096 + 17000, 4096 + 16384, 0]
    out, lengths, _ = pkg.load_batch([data] * 3, dtype=torch.int32, frame_offsets=offs, max_frames=6000)
    assert lengths.tolist() == [6000, 6000, 6000]
    for f, off in enumerate(offs):
        assert torch.equal(out[f].cpu(), w[:, off:off + 6000]), f
