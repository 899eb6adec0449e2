"""Host side of the destination mode (alacgpu_decode_into_device): argument checks of the C entry point and of its Python
wrapper, and container.packet_table on synthetic M4A files.  No GPU needed."""
import ctypes as C
import io

import numpy as np
import pytest


@pytest.fixture(scope="module")
def pkg():
    import alac.net_amd as p

    p.lib()
    return p


def _call(pkg, ctx=None, channels=2, layout=1, dtype=1, plane_stride=16, arrays=True):
    buf = (C.c_uint64 * 64)()
    vp = C.c_void_p(C.addressof(buf)) if arrays else None
    return pkg.lib().alacgpu_decode_into_device(ctx, vp, 16, vp, vp, None, 1, vp, vp, vp, 64, channels, layout, dtype,
                                                plane_stride, None, vp, None)


def test_null_ctx_and_bad_arguments_are_refused(pkg):
    assert _call(pkg) == -1                                   # a null ctx
    for kw in (dict(channels=0), dict(channels=3), dict(layout=2), dict(layout=-1), dict(dtype=2), dict(plane_stride=0),
               dict(arrays=False)):
        assert _call(pkg, **kw) == -1, kw
    assert pkg.lib().alacgpu_status_string(8).decode().startswith("destination run")
    assert pkg.ST_DEST_RANGE == 8 and (pkg.DST_INTERLEAVED, pkg.DST_PLANAR, pkg.DST_INT32, pkg.DST_FLOAT32) == (0, 1, 0, 1)


def test_decode_into_device_checks_the_output_tensor_before_any_library_call(pkg, monkeypatch):
    import torch

    calls = []
    monkeypatch.setattr(pkg, "lib", lambda: calls.append(1))
    ctx = object.__new__(pkg.AlacGpuContext)                 # (no device here: the checks come first)
    ctx._ctx = C.c_void_p()
    args = (None, 0, None, None, None, 0, None, None)
    with pytest.raises(ValueError, match="int32 or torch.float32"):
        ctx.decode_into_device(*args, torch.zeros(8, dtype=torch.float64), 2)
    with pytest.raises(ValueError, match="int32 or torch.float32"):
        ctx.decode_into_device(*args, torch.zeros(8, dtype=torch.int16), 2)
    with pytest.raises(ValueError, match="contiguous"):
        ctx.decode_into_device(*args, torch.zeros(4, 8, dtype=torch.float32).t(), 2)
    with pytest.raises(ValueError, match="device tensor"):
        ctx.decode_into_device(*args, torch.zeros(8, dtype=torch.float32), 2)
    with pytest.raises(ValueError, match="device tensor"):
        ctx.decode_into_device(*args, torch.zeros(8, dtype=torch.int32), 2, layout="interleaved")
    assert calls == []


def _file(synth, n_packets, last, stereo=True, sample_size=16, **kw):
    from alac.net_amd.synth import m4a

    d = synth.packet_descs(n_packets, sample_size=sample_size, stereo=int(stereo), pred_order=8)
    d["n"][-1] = last
    b = synth.make_batch(d, synth.default_signal(9))
    packets = [bytes(b["blob"][int(o):int(o) + int(s)]) for o, s in zip(b["offsets"], b["sizes"])]
    durs = [int(x) for x in d["n"]]
    data = m4a.write_m4a(packets, durs, sample_size=sample_size, channels=2 if stereo else 1, sample_rate=48000, **kw)
    return data, packets, durs


@pytest.mark.parametrize("kw", [{}, dict(uniform_stsz=True), dict(extra_atoms=True), dict(uniform_stsz=True, extra_atoms=True)])
def test_packet_table_gives_what_the_writer_was_given(pkg, synth, kw):
    from alac.net_amd import container

    data, packets, durs = _file(synth, 11, 777, **kw)
    if kw.get("uniform_stsz"):
        size = max(len(p) for p in packets)
        packets = [p + bytes(size - len(p)) for p in packets]
    for src in (data, io.BytesIO(data)):
        t = container.packet_table(src)
        assert t["sizes"].dtype == np.uint32 and t["sizes"].tolist() == [len(p) for p in packets]
        assert t["durations"].tolist() == durs
        assert t["dst_first"].tolist() == [sum(durs[:i]) for i in range(len(durs))]
        assert t["num_samples"] == sum(durs) == 10 * 4096 + 777
        assert (t["sample_rate"], t["num_channels"], t["sample_size"]) == (48000, 2, 16)
        for p in range(11):
            o = int(t["offsets"][p])
            assert bytes(t["blob"][o:o + int(t["sizes"][p])]) == packets[p]
        assert int(t["cfg"][0]["max_samples_per_frame"]) == 4096 and int(t["cfg"][0]["num_channels"]) == 2


def test_packet_table_mono_24bit_from_a_path(pkg, synth, tmp_path):
    from alac.net_amd import container

    data, packets, durs = _file(synth, 3, 5, stereo=False, sample_size=24)
    path = tmp_path / "m.m4a"
    path.write_bytes(data)
    t = container.packet_table(str(path))
    assert t["durations"].tolist() == [4096, 4096, 5] and t["dst_first"].tolist() == [0, 4096, 8192]
    assert (t["num_channels"], t["sample_size"]) == (1, 24) and int(t["cfg"][0]["sample_size"]) == 24
    with pytest.raises(IOError):
        container.packet_table(data.replace(b"smhd", b"vmhd"))
