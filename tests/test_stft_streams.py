"""alacgpu_stft_device on two streams: the call uses nothing of the context but its device -- no scratch, no atomics -- so two
calls with different inputs on two streams of one context are each their own single-stream result, back to back, with no host
wait between them.  The calls are made as tests/stage_stream_calls.py makes the other transforms': `transform_call`, a `Call`
whose input is loaded on the stream that runs it and whose output is cloned on it behind the call, and whose reference is the
same call alone on a fresh context."""
import pytest

from stage_stream_calls import CFG, alone, same_bits, transform_call

pytestmark = pytest.mark.gpu

ROUNDS = 16


def test_two_calls_on_two_streams_are_each_their_own():
    import torch

    import alac.net_amd as pkg

    spec = pkg.Spectrogram(2000, 256, 64, filterbank=pkg.mel_filterbank(2000, 256, 30), log="ln")
    A, B = transform_call(torch, pkg, spec, 30, seed=1), transform_call(torch, pkg, spec, 30, seed=2)
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
