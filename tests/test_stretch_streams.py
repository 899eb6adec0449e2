"""alacgpu_time_stretch_device on two streams: the analyse launch leaves the spectra of every frame in a scratch of the context
that the scan reads, and the scan's in a second one that the synthesis reads, so two calls of one context on two streams share
them one after the other (the scratch protocol of alacgpu_ctx.h) and are each their own single-stream result -- the output and
the new lengths bit for bit --, back to back for more rounds than there are launch slots, with no host wait between them and
with another stage's call, a levelling with a scratch of its own, between them on the second stream.  The first call of a
context uploads the transform's tables on its own stream; the second call, on the other stream, uses them.  The calls are made
as tests/stage_stream_calls.py makes the other stages'."""
import numpy as np
import pytest

from stage_stream_calls import CFG, Call, alone, same_bits
from test_level_streams import level_call

pytestmark = pytest.mark.gpu

ROUNDS = 24


def stretch_call(torch, seed, rows, frames, channels, terms):
    """A time stretch of rows of different lengths, every row live: the signal, the lengths and the factors are inputs the call
    reads on its stream.  The two calls differ in rows and frames, so in the scratch they need."""
    rng = np.random.default_rng(900 + seed)
    g = torch.Generator(device="cuda")
    g.manual_seed(900 + seed)
    p = [terms[b % len(terms)][0] for b in range(rows)]
    q = [terms[b % len(terms)][1] for b in range(rows)]
    true = dict(x=0.3 * torch.randn((rows, channels, frames), generator=g, device="cuda", dtype=torch.float32),
                valid=torch.from_numpy(rng.integers(frames // 2, frames + 1, rows)).to("cuda"),
                p=torch.tensor(p, dtype=torch.int32, device="cuda"), q=torch.tensor(q, dtype=torch.int32, device="cuda"))
    out_frames = max((2 * frames * a + b) // (2 * b) for a, b in terms)
    outs = [torch.empty((rows, channels, out_frames), dtype=torch.float32, device="cuda"), torch.empty(rows, dtype=torch.int64, device="cuda")]

    def fn(ctx, b, o, stream):
        ctx.time_stretch_device(b["x"], o[0], rows, channels, frames, out_frames, frames, out_frames, b["p"], b["q"], b["valid"], o[1],
                                512, stream=stream)

    return Call(torch, true, outs, fn, wrong=dict(valid=frames, p=1, q=1))


def test_two_calls_on_two_streams_are_each_their_own():
    import torch

    import alac.net_amd as pkg

    A = stretch_call(torch, 1, rows=5, frames=3000, channels=2, terms=((11, 10), (9, 10), (2, 1)))
    B = stretch_call(torch, 2, rows=3, frames=5000, channels=1, terms=((1, 2), (200, 189)))
    Lv = level_call(torch, pkg, 3, rows=3, frames=9000)
    wantA, wantB, wantL = alone(torch, pkg, A), alone(torch, pkg, B), alone(torch, pkg, Lv)
    assert bool(torch.isfinite(wantA[0]).all()) and bool(torch.isfinite(wantB[0]).all())      # every row is live and wholly written
    assert bool((wantA[1] > 0).all()) and bool((wantB[1] > 0).all())
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with pkg.AlacGpuContext(CFG) as ctx:
        gotA, gotB, gotL = [], [], []
        for _ in range(ROUNDS):
            for call, s, got in ((A, s1, gotA), (B, s2, gotB), (Lv, s2, gotL)):
                with torch.cuda.stream(s):
                    call.poison()
                    call.load()
                    call.run(ctx, s.cuda_stream)
                    got.append(call.clones())
        torch.cuda.synchronize()
    for r in range(ROUNDS):
        assert same_bits(torch, gotA[r], wantA) and same_bits(torch, gotB[r], wantB) and same_bits(torch, gotL[r], wantL), r
