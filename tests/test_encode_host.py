"""alac.net_amd.save / save_batch on the host: the argument checks run before any device work, and the M4A writer (now in
the product package) with the cookie's maxFrameBytes / avgBitRate."""
import hashlib
import struct

import pytest


@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to open a GPU context fails the test: every error below must come before device work."""
    import alac.net_amd as pkg

    def boom(*a, **k):
        raise AssertionError("device work before the argument checks")

    monkeypatch.setattr(pkg, "AlacGpuContext", boom)
    return pkg


def meta(shape, dtype=None):
    import torch

    return torch.empty(shape, dtype=dtype or torch.int32, device="meta")


@pytest.mark.parametrize("shape,kw,match", [
    ((3, 100), {}, "channels"),
    ((0, 100), {}, "channels"),
    ((2, 100), {"sample_size": 20}, "sample_size"),
    ((2, 100), {"sample_size": 32}, "sample_size"),
    ((2, 100), {"frame_length": 0}, "frame_length"),
    ((2, 100), {"frame_length": 16385}, "frame_length"),
    ((2, 0), {}, "empty"),
    ((2, 100, 3), {}, "shape"),
    ((1, 1 << 31), {}, "stco"),
    ((2, 1 << 30), {"sample_size": 24}, "stco"),
])
def test_save_refuses_before_device_work(no_device, shape, kw, match):
    with pytest.raises(ValueError, match=match):
        no_device.save("unused.m4a", meta(shape), 44100, **kw)


def test_save_refuses_host_and_other_dtypes(no_device):
    import torch

    with pytest.raises(ValueError, match="GPU"):
        no_device.save("unused.m4a", torch.zeros((2, 10), dtype=torch.int32), 44100)
    with pytest.raises(ValueError, match="GPU"):
        no_device.save("unused.m4a", meta((1, 4096)), 44100)
    with pytest.raises(ValueError, match="int32 or torch.float32"):
        no_device.save("unused.m4a", meta((2, 10), torch.int16), 44100)
    with pytest.raises(ValueError, match="sample_rate"):
        no_device.save("unused.m4a", meta((2, 10)), 0)


def test_save_batch_refuses_before_device_work(no_device):
    with pytest.raises(ValueError, match="shape"):
        no_device.save_batch(["a"], meta((2, 10)), [10], 44100)
    with pytest.raises(ValueError, match="channels"):
        no_device.save_batch(["a"], meta((1, 3, 10)), [10], 44100)
    with pytest.raises(ValueError, match="empty"):
        no_device.save_batch([], meta((0, 2, 10)), [], 44100)
    with pytest.raises(ValueError, match="destinations"):
        no_device.save_batch(["a"], meta((2, 2, 10)), [10, 10], 44100)
    with pytest.raises(ValueError, match="length"):
        no_device.save_batch(["a", "b"], meta((2, 2, 10)), [10, 11], 44100)
    with pytest.raises(ValueError, match="length"):
        no_device.save_batch(["a", "b"], meta((2, 2, 10)), [10, 0], 44100)
    with pytest.raises(ValueError, match="stco"):
        no_device.save_batch(["a", "b"], meta((2, 2, 1 << 30)), [10, 1 << 30], 44100)
    with pytest.raises(ValueError, match="GPU"):
        no_device.save_batch(["a", "b"], meta((2, 2, 10)), [10, 3], 44100)


def test_encode_max_packet_bytes():
    import alac.net_amd as pkg

    # an escape packet with its sample count: 23 + 32 header bits, the samples, 3 END bits; rounded up to 16 bytes
    for frames, ss, ch in [(4096, 16, 2), (4096, 24, 2), (1, 16, 1), (16384, 24, 2), (1000, 24, 1)]:
        bits = 23 + 32 + frames * ch * ss + 3
        assert pkg.encode_max_packet_bytes(frames, ss, ch) == -(-(-(-bits // 8)) // 16) * 16


PACKETS = [bytes((i * 7 + j) & 0xFF for j in range(40 + 13 * i)) for i in range(12)]
DURATIONS = [4096] * 11 + [1000]


@pytest.mark.parametrize("kw,digest", [
    ({}, "865299c9659c7604e275c24c0d0520ab73d5d6a69aabf8fb6354b8fbd6a438d2"),
    ({"packets_per_chunk": 3}, "01a64460b9373b5d091dae4ed2af8f1fe83fb5294de6888d4dee7228898c2822"),
    ({"mdat_first": True}, "08e2ef2872d725fcb52229d4b2168ef1a6bb61e89da8cf7e19f4fd315b1f0ac8"),
    ({"uniform_stsz": True}, "c5c6c807ca7c237d4d361c97353b9940ec7e034a100921bf71a9d47adf30b069"),
    ({"extra_atoms": True}, "0978161e77b45eb72884abd5fb118b62c8ce70282656a9b86e70b7ae33a61c7e"),
    ({"sample_size": 24, "channels": 1, "sample_rate": 48000, "pb": 20, "mb": 11, "kb": 15},
     "e8038822ae8414fdd3dbca13ce093fe0ee3705ed49d62fd9a47cc31ae38146dd"),
])
def test_writer_output_is_unchanged_under_both_imports(kw, digest):
    """The digests are of the writer's output before it moved into the product package."""
    from alac.net_amd import container
    from alac.net_amd.synth import m4a

    a = m4a.write_m4a(PACKETS, DURATIONS, **kw)
    assert hashlib.sha256(a).hexdigest() == digest
    assert container.write_m4a(PACKETS, DURATIONS, **kw) == a


def alac_cookie(data):
    """The 24-byte ALACSpecificConfig of the file's sample description (the inner `alac` atom)."""
    at = data.rfind(b"alac")
    size = struct.unpack(">I", data[at - 4:at])[0]
    assert size == 36
    return struct.unpack(">IBBBBBBHIII", data[at + 8:at + 32])


def test_writer_cookie_max_frame_bytes_and_avg_bitrate():
    from alac.net_amd import container

    data = container.write_m4a(PACKETS, DURATIONS, max_frame_bytes=183, avg_bitrate=705600, sample_rate=48000)
    (frame_len, _, ss, pb, mb, kb, ch, maxrun, max_frame_bytes, avg_bitrate, rate) = alac_cookie(data)
    assert (frame_len, ss, pb, mb, kb, ch, maxrun, rate) == (4096, 16, 40, 10, 14, 2, 255, 48000)
    assert (max_frame_bytes, avg_bitrate) == (183, 705600)
    assert alac_cookie(container.write_m4a(PACKETS, DURATIONS))[8:10] == (0, 0)   # defaults stay 0
    t = container.packet_table(data)     # the demuxer reads the file as before
    assert t["sizes"].tolist() == [len(p) for p in PACKETS] and t["num_samples"] == sum(DURATIONS)
