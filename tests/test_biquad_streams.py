"""alacgpu_biquad_device on two streams: the call uses nothing of the context but its device -- no scratch, no atomics -- so two
calls with different inputs on two streams of one context are each their own single-stream result, back to back for more rounds
than there are launch slots, with no host wait between them.  The calls are made as tests/stage_stream_calls.py makes the other
stages': a `Call` whose inputs are loaded on the stream that runs it, and whose reference is the same call alone on a fresh
context."""
import numpy as np
import pytest

from stage_stream_calls import CFG, Call, alone, same_bits

pytestmark = pytest.mark.gpu

ROUNDS = 32


def biquad_call(torch, pkg, seed, rows=5, channels=2, frames=9000, sections=4):
    """A biquad call out of place over rows of different lengths: the signal, the lengths, the coefficients and the gains are
    all inputs the call reads on its stream"""
    from test_biquad_spec import stable_sections

    rng = np.random.default_rng(300 + seed)
    g = torch.Generator(device="cuda")
    g.manual_seed(300 + seed)
    true = dict(x=0.1 * torch.randn((rows, channels, frames), generator=g, device="cuda", dtype=torch.float32),
                valid=torch.from_numpy(rng.integers(1, frames + 1, rows)).to("cuda"),
                coeffs=torch.from_numpy(stable_sections(rng, (rows, sections))).to("cuda"),
                gain=torch.from_numpy(rng.uniform(0.125, 2.0, rows)).to("cuda"))
    outs = [torch.empty((rows, channels, frames), dtype=torch.float32, device="cuda")]

    def fn(ctx, b, o, stream):
        ctx.biquad_device(b["x"], o[0], rows, channels, frames, frames, b["valid"], b["coeffs"], sections, b["gain"], True, stream=stream)

    return Call(torch, true, outs, fn, wrong=dict(valid=frames))


def test_two_calls_on_two_streams_are_each_their_own():
    import torch

    import alac.net_amd as pkg

    A, B = biquad_call(torch, pkg, 1), biquad_call(torch, pkg, 2)
    wantA, wantB = alone(torch, pkg, A), alone(torch, pkg, B)
    assert not same_bits(torch, wantA, wantB)
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
