"""window_plan (the packets of a frame window, on the host) against a brute-force per-frame mapping, and the ValueErrors of
load / load_batch / info that come before any device work.  CPU only."""
import numpy as np
import pytest


def owner_map(durations, offset, length):
    """Brute force: for each window frame, its packet and its frame inside the packet (frame t belongs to the packet p with
    dst_first[p] <= t < dst_first[p] + durations[p])."""
    pk = np.repeat(np.arange(len(durations)), durations)
    inner = np.concatenate([np.arange(d) for d in durations]) if len(durations) else np.zeros(0, np.int64)
    return pk[offset:offset + length], inner[offset:offset + length]


def check_plan(durations, offset, length):
    import alac.net_amd as pkg

    durations = np.asarray(durations, dtype=np.int64)
    dst_first = np.concatenate([[0], np.cumsum(durations)[:-1]]).astype(np.int64) if len(durations) else np.zeros(0, np.int64)
    p0, p1, first, frames, skip = pkg.window_plan(dst_first, durations, offset, length)
    assert len(first) == len(frames) == len(skip) == p1 - p0
    assert (frames >= 0).all() and (skip >= 0).all() and (first >= 0).all()
    pk = np.full(length, -1, dtype=np.int64)
    inner = np.full(length, -1, dtype=np.int64)
    for k in range(p1 - p0):
        w = first[k] + np.arange(frames[k])
        assert (pk[w] == -1).all(), "a window frame placed twice"
        pk[w] = p0 + k
        inner[w] = skip[k] + np.arange(frames[k])
        assert skip[k] + frames[k] <= durations[p0 + k]
    want_pk, want_inner = owner_map(durations, offset, length)
    assert np.array_equal(pk, want_pk) and np.array_equal(inner, want_inner)
    # the range is the smallest contiguous one: its first and last packets hold window frames
    if length:
        assert frames[-1] > 0 and (frames[0] > 0 or offset == 0)
        assert p0 == 0 or offset > 0
    else:
        assert p1 == p0
    return p0, p1, first, frames, skip


def test_random_windows_against_brute_force():
    rng = np.random.default_rng(11)
    for trial in range(300):
        n = int(rng.integers(1, 40))
        durations = rng.choice([4096, 4096, 4096, 1, 17, 1000, 16384, 0], size=n)
        if trial % 3 == 0:
            durations[:] = 4096
            durations[-1] = int(rng.integers(1, 4097))      # a short last packet
        T = int(durations.sum())
        offset = int(rng.integers(0, T + 1))
        length = int(rng.integers(0, T - offset + 1))
        check_plan(durations, offset, length)


def test_offsets_on_and_next_to_packet_boundaries():
    durations = np.array([4096, 4096, 1000, 4096, 1234])
    T = int(durations.sum())
    bounds = np.concatenate([[0], np.cumsum(durations)])
    for b in bounds:
        for o in (b - 1, b, b + 1):
            if 0 <= o <= T:
                for length in (0, 1, 2, 4095, 4096, 4097, T - o):
                    if 0 <= length <= T - o:
                        check_plan(durations, int(o), int(length))
    # on a boundary: no skip, the window starts with that packet
    p0, p1, first, frames, skip = check_plan(durations, 8192, 100)
    assert (p0, p1) == (2, 3) and skip.tolist() == [0] and frames.tolist() == [100] and first.tolist() == [0]
    # one frame past it: the packet is skipped into
    p0, p1, first, frames, skip = check_plan(durations, 8193, 5000)
    assert (p0, p1) == (2, 4) and skip.tolist() == [1, 0] and frames.tolist() == [999, 4001] and first.tolist() == [0, 999]
    # inside the short last packet, and the window that ends there
    p0, p1, first, frames, skip = check_plan(durations, T - 10, 10)
    assert (p0, p1) == (4, 5) and skip.tolist() == [1224] and frames.tolist() == [10]


def test_irregular_durations_and_empty_windows():
    durations = np.array([0, 3, 0, 0, 5, 16384, 0, 2, 0])
    T = int(durations.sum())
    bounds = np.concatenate([[0], np.cumsum(durations)])
    near = sorted({int(b) + d for b in bounds for d in (-2, -1, 0, 1, 2)} | set(range(0, 12)) | set(range(T - 12, T + 1)))
    for o in [o for o in near if 0 <= o <= T]:
        for length in range(0, min(T - o, 20) + 1):
            check_plan(durations, o, length)
    # from frame 0 the window starts at packet 0 (what load_batch always took); packets without frames at its end stay out
    p0, p1, _, frames, _ = check_plan(durations, 0, T)
    assert (p0, p1) == (0, 8) and frames.tolist() == [0, 3, 0, 0, 5, 16384, 0, 2]
    assert check_plan(durations, T, 0)[:2] == (0, 0)
    assert check_plan(durations, 3, 0)[:2] == (0, 0)
    assert check_plan([], 0, 0)[:2] == (0, 0)


def test_plan_refuses_negative_arguments():
    import alac.net_amd as pkg

    with pytest.raises(ValueError):
        pkg.window_plan([0], [10], -1, 5)
    with pytest.raises(ValueError):
        pkg.window_plan([0], [10], 0, -5)


def small_file(synth, n_packets=3, last=100):
    from alac.net_amd.synth import m4a

    d = synth.packet_descs(n_packets, stereo=1)
    d["n"][-1] = last
    b = synth.make_batch(d, synth.default_signal(3))
    packets = [bytes(b["blob"][int(o):int(o) + int(s)]) for o, s in zip(b["offsets"], b["sizes"])]
    return m4a.write_m4a(packets, [int(x) for x in d["n"]], sample_size=16, channels=2, sample_rate=48000)


def test_info_reads_the_headers_only(synth, tmp_path):
    import alac.net_amd as pkg
    from alac.net_amd import container

    data = small_file(synth)
    want = dict(num_frames=2 * 4096 + 100, channels=2, sample_rate=48000, sample_size=16)
    assert pkg.info(data) == want
    path = tmp_path / "a.m4a"
    path.write_bytes(data)
    assert pkg.info(str(path)) == want
    with open(path, "rb") as f:
        assert pkg.info(f) == want
    t, h = container.packet_table(data), container.header_table(data)
    assert np.array_equal(t["sizes"], h["sizes"]) and np.array_equal(t["durations"], h["durations"])
    assert all(t[k] == h[k] for k in ("sample_rate", "num_channels", "sample_size", "num_samples"))
    with pytest.raises(ValueError):
        pkg.info(12345)
    with pytest.raises(IOError):
        pkg.info(data.replace(b"smhd", b"vmhd"))


def test_bad_windows_raise_before_any_device_work(synth):
    # every one of these is refused on the host: no GPU is needed to see the ValueError
    import alac.net_amd as pkg

    data = small_file(synth)
    T = 2 * 4096 + 100
    for kw in (dict(frame_offset=-1), dict(frame_offset=T + 1), dict(num_frames=-1), dict(frame_offset=1.5),
               dict(frame_offset=0, num_frames=-3)):
        with pytest.raises(ValueError):
            pkg.load(data, **kw)
    with pytest.raises(ValueError):
        pkg.load_batch([data, data], frame_offsets=[0])
    with pytest.raises(ValueError):
        pkg.load_batch([data, data], frame_offsets=[0, T + 1])
    with pytest.raises(ValueError, match="source 1"):
        pkg.load_batch([data, small_file(synth, 2, 5)], frame_offsets=4096 + 6)
    with pytest.raises(ValueError):
        pkg.load_batch([data], frame_offsets=-2)
    with pytest.raises(ValueError):
        pkg.load_batch([data], frame_offsets=[-2])
