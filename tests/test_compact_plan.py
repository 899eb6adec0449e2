"""The packet compaction's host side: compact_plan_host (the kernel's specification), the entry point's declaration, binding
and argument checks, and Corpus.from_pcm's refusals -- none of it needs a GPU."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_compact_plan_host():
    import alac.net_amd as pkg

    sizes = np.array([5, 0, 16, 17, 3, 2 ** 32 - 1, 16, 0, 1], dtype=np.uint32)
    off, total, copied = pkg.compact_plan_host(sizes, 16, 7, 10 ** 9)
    # 17 and 2^32 - 1 are above the slot: they count as 0
    counted = [5, 0, 16, 0, 3, 0, 16, 0, 1]
    assert off.dtype == np.uint64 and off.tolist() == [7 + sum(counted[:i]) for i in range(9)]
    assert total == sum(counted) == 41 and copied.dtype == bool and copied.all()
    # the capacity cuts in the middle of packet 2 (bytes 12 .. 28): it and every packet with bytes behind it are absent;
    # packets without bytes "fit" wherever their offset does.  total ignores the capacity
    off2, total2, copied2 = pkg.compact_plan_host(sizes, 16, 7, 20)
    assert off2.tolist() == off.tolist() and total2 == 41
    assert copied2.tolist() == [o + c <= 20 for o, c in zip(off.tolist(), counted)] == [True, True] + [False] * 7
    assert pkg.compact_plan_host(sizes, 16, 7, 28)[2].tolist() == [True, True, True, True, False, False, False, False, False]
    assert not pkg.compact_plan_host(sizes, 16, 7, 0)[2].any()
    # slot_bytes itself is a size that counts
    assert pkg.compact_plan_host([48, 49], 48, 0, 100)[1] == 48
    # offsets are 64-bit: a base above 4 GiB, sizes that sum past it
    big = np.full(300000, 16000, dtype=np.uint32)
    off, total, copied = pkg.compact_plan_host(big, 16400, 1 << 33, 1 << 62)
    assert total == 300000 * 16000 > 1 << 32 and int(off[-1]) == (1 << 33) + 299999 * 16000 and copied.all()
    rng = np.random.default_rng(1)
    s = rng.integers(0, 60, 1000).astype(np.uint32)
    off, total, _ = pkg.compact_plan_host(s, 48, 3, 0)
    c = np.where(s <= 48, s, 0).astype(np.int64)
    assert np.array_equal(off.astype(np.int64), 3 + np.cumsum(c) - c) and total == int(c.sum())
    # n = 0
    off, total, copied = pkg.compact_plan_host(np.zeros(0, np.uint32), 16, 5, 100)
    assert len(off) == 0 and off.dtype == np.uint64 and total == 0 and len(copied) == 0 and copied.dtype == bool


def test_the_entry_point_is_declared_bound_and_exported():
    import alac.net_amd as pkg

    src = open(os.path.join(ROOT, "include", "alacgpu.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"int\s+alacgpu_compact_packets_device\s*\(([^)]*)\)", src)
    assert m, "include/alacgpu.h does not declare alacgpu_compact_packets_device"
    assert len(m.group(1).split(",")) == len(pkg.SYMBOLS["alacgpu_compact_packets_device"][1]) == 11
    assert hasattr(pkg.lib(), "alacgpu_compact_packets_device")
    assert hasattr(pkg.AlacGpuContext, "compact_packets_device")
    cs = open(os.path.join(ROOT, "alac.net_amd", "host", "csharp", "AlacGpuNative.cs")).read()
    assert "alacgpu_compact_packets_device(" in cs
    # argument checks come before any device work
    assert pkg.lib().alacgpu_compact_packets_device(None, None, 16, None, 1, None, 0, 0, None, None, None) == -1
    assert pkg.lib().alacgpu_compact_packets_device(None, None, 16, None, 0, None, 0, 0, None, None, None) == -1


def test_from_pcm_refuses_before_any_device_work():
    import torch

    import alac.net_amd as pkg


    ok = torch.zeros((2, 2, 100), dtype=torch.int32)
    with pytest.raises(ValueError, match="on the GPU"):
        pkg.Corpus.from_pcm(ok, [100, 50], 44100)
    with pytest.raises(ValueError, match="3 channels"):
        pkg.Corpus.from_pcm(torch.zeros((2, 3, 100), dtype=torch.int32), [100, 50], 44100)
    with pytest.raises(ValueError, match="sample_size"):
        pkg.Corpus.from_pcm(ok, [100, 50], 44100, sample_size=20)
    for fl in (0, 16385):
        with pytest.raises(ValueError, match="frame_length"):
            pkg.Corpus.from_pcm(ok, [100, 50], 44100, frame_length=fl)
    with pytest.raises(ValueError, match="length 101"):
        pkg.Corpus.from_pcm(ok, [100, 101], 44100)
    with pytest.raises(ValueError, match="lengths"):
        pkg.Corpus.from_pcm(ok, [100], 44100)
    with pytest.raises(ValueError, match="sample_rate"):
        pkg.Corpus.from_pcm(ok, [100, 50])
    with pytest.raises(ValueError, match="no sources"):
        pkg.Corpus.from_pcm([], sample_rate=44100)
    with pytest.raises(ValueError, match="no sources"):
        pkg.Corpus.from_pcm(iter(()), sample_rate=44100)
    # a batch of an iterable is checked as a single one is
    with pytest.raises(ValueError, match="on the GPU"):
        pkg.Corpus.from_pcm([(ok, [100, 50])], sample_rate=44100)
    with pytest.raises(ValueError, match="3 channels"):
        pkg.Corpus.from_pcm(iter([(torch.zeros((1, 3, 8), dtype=torch.int32), [8])]), sample_rate=44100)
