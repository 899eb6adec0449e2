"""alacgpu_level_device on two streams: the measure launch leaves the sums of every plane in a scratch of the context that the
apply launch reads, so two calls of one context on two streams share it one after the other (the scratch protocol of
alacgpu_ctx.h) and are each their own single-stream result -- the output, g, E and P bit for bit --, back to back for more
rounds than there are launch slots, with no host wait between them.  The calls are made as tests/stage_stream_calls.py makes
the other stages'."""
import sys

import numpy as np
import pytest

from stage_stream_calls import CFG, Call, alone, same_bits

pytestmark = pytest.mark.gpu

ROUNDS = 24


def level_call(torch, pkg, seed, rows, frames, rate=8000, channels=2):
    """A loudness levelling out of place over rows of different lengths and levels, with its three outputs: the signal and the
    lengths are inputs the call reads on its stream.  The two calls differ in rows and frames, so in the scratch they need."""
    lv = sys.modules["alac.net_amd.level"]
    rng = np.random.default_rng(700 + seed)
    g = torch.Generator(device="cuda")
    g.manual_seed(700 + seed)
    amp = torch.from_numpy(rng.uniform(0.01, 0.5, rows).astype(np.float32)).to("cuda")
    true = dict(x=amp[:, None, None] * torch.randn((rows, channels, frames), generator=g, device="cuda", dtype=torch.float32),
                valid=torch.from_numpy(rng.integers(4 * 800, frames + 1, rows)).to("cuda"))
    outs = [torch.empty((rows, channels, frames), dtype=torch.float32, device="cuda")] + [
        torch.empty(rows, dtype=torch.float64, device="cuda") for _ in range(3)]
    spec = lv.Level.lufs(-20.0, max_peak=0.99, clamp=True)
    q = lv._kweight_device(float(rate), "cuda:0")

    def fn(ctx, b, o, stream):
        ctx.level_device(b["x"], o[0], rows, channels, frames, frames, b["valid"], lv.LUFS, lv.hop_frames(rate), q, spec.linear, spec.max_peak,
                         spec.clamp, o[1], o[2], o[3], stream=stream)

    return Call(torch, true, outs, fn, wrong=dict(valid=frames), keep=q)


def test_two_calls_on_two_streams_are_each_their_own():
    import torch

    import alac.net_amd as pkg

    A, B = level_call(torch, pkg, 1, rows=5, frames=9000), level_call(torch, pkg, 2, rows=3, frames=20000)
    wantA, wantB = alone(torch, pkg, A), alone(torch, pkg, B)
    assert bool((wantA[1] != 1.0).all()) and bool((wantB[1] != 1.0).all())            # every row is measured and levelled
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with pkg.AlacGpuContext(CFG) as ctx:
        gotA, gotB = [], []
        for _ in range(ROUNDS):
            for call, s, got in ((A, s1, gotA), (B, s2, gotB)):
                with torch.cuda.stream(s):
                    call.poison()
                    call.load()
                    call.run(ctx, s.cuda_stream)
                    got.append(call.clones())
        torch.cuda.synchronize()
    for r in range(ROUNDS):
        assert same_bits(torch, gotA[r], wantA) and same_bits(torch, gotB[r], wantB), r
